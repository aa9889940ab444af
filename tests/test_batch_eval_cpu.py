"""CPU tests of the training-batch evaluator (include/yolo355.h: y3_batch_eval): the per-cell and per-detection functions
the kernels are made of (csrc/y3_beval_px.h) run on the host (tests/beval_emul.cpp) against eval_utils._evaluate over every
case of tests/beval_cases.py; exact integer equality of the three per-class count vectors, no tolerance.  Plus the
interface: prototypes, build list, scratch size, argument validation before any launch, train.py's flag.
tests/test_batch_eval_gpu.py repeats the comparison with the kernels themselves."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import beval_cases as bc

SIZES = [(160, 128), (128, 160)]
CLASSES = [1, 3, 80]


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('beval_emul') / 'libbeval_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-Wall',
                           os.path.join(ROOT, 'tests', 'beval_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3be_emulate.restype = ctypes.c_int
    lib.y3be_emulate.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [
        ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emulate(emul, case, table=None):
    """(table int64 [C, 3], overflow word) of one case through the host build."""
    table = np.zeros((case.class_num, 3), np.int64) if table is None else table
    state = np.zeros(1, np.int32)
    y = [np.ascontiguousarray(t) for t in case.y_true]
    gt_cap = case.gt_cap if case.gt_cap is not None else min(bc.cells_of_image(case.h, case.w), 4096)
    p = lambda x: x.ctypes.data
    assert emul.y3be_emulate(p(case.boxes), p(case.labels), p(case.counts), len(case.counts), case.boxes.shape[1], p(y[0]), p(y[1]),
                             p(y[2]), case.h, case.w, case.class_num, case.iou_thresh, gt_cap, p(table), p(state)) == 0
    return table, int(state[0])


def test_the_interface_exists():
    """The C entries, their prototypes, the build list and the Python entry (this is what fails on a tree without the feature)."""
    from yolov3_tensorflow_amd import _lib, build
    from yolov3_tensorflow_amd.utils import eval_utils
    for name in ('y3_batch_eval', 'y3_batch_eval_scratch_bytes'):
        assert name in _lib.PROTOTYPES
    assert ('y3_beval.hip', ['-ffp-contract=off']) in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'y3_beval_px.h'))
    header = open(os.path.join(ROOT, 'include', 'yolo355.h')).read()
    assert 'int y3_batch_eval(' in header and 'size_t y3_batch_eval_scratch_bytes(int n, int gt_cap);' in header
    assert '#define Y3_ABI_VERSION 5' in header
    assert callable(eval_utils.evaluate_on_device)


def test_scratch_bytes_and_validation_before_launching():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    size = L.y3_batch_eval_scratch_bytes
    assert size(0, 8) == 0 and size(8, 0) == 0 and size(-1, 8) == 0 and size(8, -3) == 0
    assert size(1, 1) >= 32 + 4 + 4 + 4
    assert size(2, 100) == 8704 and size(1, 1) == 1024 and size(5, 70) == 14592 and size(64, 4096) == 10486016
    for n, g in ((1, 1), (5, 70), (64, 4096)):
        assert size(n, g) >= n * g * (32 + 4) + n * 4
        assert size(n + 1, g) >= size(n, g) and size(n, g + 1) >= size(n, g)
        if n * g >= 64:      # (sizes are rounded up to 256 bytes: strictly more only beyond the rounding)
            assert size(2 * n, g) > size(n, g) and size(n, 2 * g + 64) > size(n, g)
    d = ctypes.c_void_p(4096)
    big = 1 << 40
    call = lambda ctx=d, ob=d, ol=d, cnt=d, n=2, cap=8, y1=d, y2=d, y3=d, h=64, w=96, C=3, thr=0.5, gt_cap=16, ws=d, wsb=big, \
        table=d, state=d: L.y3_batch_eval(ctx, ob, ol, cnt, n, cap, y1, y2, y3, h, w, C, thr, gt_cap, ws, wsb, table, state)
    for null in ('ctx', 'ob', 'ol', 'cnt', 'y1', 'y2', 'y3', 'ws', 'table', 'state'):
        assert call(**{null: None}) == _lib.Y3_EINVAL, null
    for name in ('n', 'cap', 'h', 'w', 'C', 'gt_cap'):
        for bad in (0, -4):
            assert call(**{name: bad}) == _lib.Y3_EINVAL, (name, bad)
    assert call(h=48) == _lib.Y3_EINVAL and call(w=100) == _lib.Y3_EINVAL and call(h=16) == _lib.Y3_EINVAL
    assert call(wsb=size(2, 16) - 1) == _lib.Y3_EINVAL and call(wsb=0) == _lib.Y3_EINVAL
    assert b'scratch too small' in L.y3_last_error()
    assert call(n=1 << 16, cap=1 << 16) == _lib.Y3_EINVAL                  # n * cap
    assert call(n=1 << 15, gt_cap=1 << 16) == _lib.Y3_EINVAL               # n * gt_cap
    assert call(n=1 << 12, h=1 << 12, w=1 << 12) == _lib.Y3_EINVAL         # n * cells
    assert call(C=(1 << 31) - 6) == _lib.Y3_EINVAL and call(C=1 << 22) == _lib.Y3_EINVAL      # channels, a pass's floats
    assert b'y3_batch_eval' in L.y3_last_error()


def test_train_parser_knows_the_flag():
    sys.path.insert(0, ROOT)
    import train as train_script
    parser = train_script.build_parser()
    assert parser.parse_args([]).batch_eval_on_device is False
    assert parser.parse_args(['--batch_eval_on_device', 'true']).batch_eval_on_device is True


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_every_case_against_evaluate(emul, size, C):
    cases = bc.all_cases(size[0], size[1], C)
    assert len(cases) >= 16
    for name, case in sorted(cases.items()):
        got, dropped = emulate(emul, case)
        assert dropped == case.dropped, name
        if case.dropped:
            continue
        want = bc.reference_of(case)
        np.testing.assert_array_equal(got, want, err_msg=name)
        if case.expect is not None:
            assert tuple(want.sum(axis=0)) == case.expect, name


def test_the_corner_cases_separate_what_they_are_built_to_separate():
    """With three classes: the tally depends on gather order, on the label check coming after the argmax, on strict >."""
    cases = bc.all_cases(160, 128, 3)
    for name in ('argmax_before_label', 'tie_across_scales', 'tie_inside_a_scale', 'one_hit_per_object', 'strict_at_threshold',
                 'strict_below_threshold', 'f32_area_at_threshold', 'f32_area_below_threshold', 'nan_box', 'empty_images',
                 'only_detections', 'only_objects', 'mix_up_cells'):
        assert cases[name].expect is not None and tuple(bc.reference_of(cases[name]).sum(axis=0)) == cases[name].expect, name
    per_class = bc.reference_table(cases['tie_across_scales'])
    assert per_class[0].tolist() == [1, 2, 2] and per_class[1].tolist() == [0, 2, 0]      # the class-0 object wins only when first
    many = cases['seventy_objects']
    assert bc.reference_of(many)[:, 1].sum() == 80 and 20 < bc.reference_of(many)[:, 0].sum() < 70


def test_recall_and_precision_and_accumulation(emul):
    """calc_now=True's two floats from the table, bit for bit; two batches into one table = the sum of two tables."""
    a, b = bc.all_cases(128, 160, 3)['random_n5_seed3'], bc.all_cases(128, 160, 3)['seventy_objects']
    for case in (a, b):
        t, _ = emulate(emul, case)
        want = bc.reference_recall_precision(case)
        got = (t[:, 0].sum() / (t[:, 1].sum() + 1e-6), t[:, 0].sum() / (t[:, 2].sum() + 1e-6))
        assert got[0].tobytes() == np.float64(want[0]).tobytes() and got[1].tobytes() == np.float64(want[1]).tobytes()
    both, _ = emulate(emul, a)
    both, _ = emulate(emul, b, table=both)
    np.testing.assert_array_equal(both, bc.reference_of(a) + bc.reference_of(b))
