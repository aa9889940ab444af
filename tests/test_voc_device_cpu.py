"""CPU tests of the device VOC evaluator's arithmetic (include/yolo355.h: y3_voc_match / y3_voc_ap): the per-detection and
per-rank functions the kernels are made of (csrc/y3_voc_px.h) run on the host (tests/voc_emul.cpp) against
eval_utils.voc_eval - the committed reference vectors, seeded random sets and the corner cases of the matching rule.
tests/test_voc_device_gpu.py repeats the comparison with the kernels themselves."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import voc_cases as vc

THRESHOLDS = np.arange(0., 1.1, 0.1)


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('voc_emul') / 'libvoc_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math',
                           os.path.join(ROOT, 'tests', 'voc_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3v_emulate.restype = ctypes.c_int
    lib.y3v_emulate.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [
        ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 4
    return lib


def emulate(emul, case, iou_thres=0.5, use_07_metric=False):
    a = vc.arena_of(case)
    rows = len(case.preds)
    out = np.full((case.class_num, 5), -7., np.float64)
    order, tp = np.full(rows, -1, np.int32), np.full(rows, 9, np.uint8)
    p = lambda x: x.ctypes.data
    assert emul.y3v_emulate(p(a['box']), p(a['score']), p(a['label']), p(a['image']), rows, p(a['gt_start']), p(a['gt_box']),
                            p(a['gt_label']), a['num_images'], a['num_gt'], case.class_num, iou_thres, int(use_07_metric),
                            p(THRESHOLDS), p(out), p(order), p(tp)) == 0
    return out, order, tp


def test_the_device_interface_exists():
    """The C entries, their prototypes and DeviceEval (this is what fails on a tree without the feature)."""
    from yolov3_tensorflow_amd import _lib
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    from yolov3_tensorflow_amd import build
    for name in ('y3_voc_append', 'y3_voc_match', 'y3_voc_ap', 'y3_voc_match_scratch_bytes', 'y3_voc_ap_scratch_bytes',
                 'y3_voc_ap_pass'):
        assert name in _lib.PROTOTYPES
    assert ('y3_voc.hip', ['-ffp-contract=off']) in build.SOURCES
    assert 'stable' in DeviceEval.__doc__
    with pytest.raises(ValueError):
        DeviceEval({1: []}, [1, 2], 3)          # (raised before anything touches a device)


def test_host_entry_points_validate_before_launching():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert L.y3_voc_ap_pass() >= 256 and L.y3_voc_ap_pass() % 64 == 0
    assert L.y3_voc_match_scratch_bytes(0, 5) == 0 and L.y3_voc_ap_scratch_bytes(0) == 0
    assert L.y3_voc_match_scratch_bytes(1000, 45) >= 1000 * 4 + 45 * 4 and L.y3_voc_ap_scratch_bytes(1000) >= 4000
    assert L.y3_voc_match_scratch_bytes(1000, 45) == 4352 and L.y3_voc_ap_scratch_bytes(1000) == 4096
    assert L.y3_voc_match_scratch_bytes(7, 0) == 512
    d = ctypes.c_void_p(4096)
    assert L.y3_voc_append(None, d, d, d, d, d, 1, 1, d, d, d, d, 1, d) == _lib.Y3_EINVAL
    assert L.y3_voc_append(d, d, d, d, d, d, 0, 1, d, d, d, d, 1, d) == _lib.Y3_EINVAL
    assert L.y3_voc_append(d, d, d, d, d, d, 1, 1, d, d, d, d, 0, d) == _lib.Y3_EINVAL
    assert L.y3_voc_append(d, d, d, d, d, d, 1 << 20, 1 << 20, d, d, d, d, 1, d) == _lib.Y3_EINVAL
    assert L.y3_voc_match(d, d, d, d, d, 8, None, d, d, d, 1, 1, 1, 0.5, d, 16, d, d) == _lib.Y3_EINVAL      # scratch too small
    assert L.y3_voc_match(d, d, d, d, d, 0, None, d, d, d, 1, 1, 1, 0.5, d, 1 << 20, d, d) == _lib.Y3_EINVAL
    assert L.y3_voc_ap(d, d, d, 8, d, 1, 1, 1, None, d, 1 << 20, d) == _lib.Y3_EINVAL                        # 11 points, no thresholds
    assert L.y3_voc_ap(d, d, d, 8, d, 1, 0, 0, None, d, 1 << 20, d) == _lib.Y3_EINVAL
    assert L.y3_voc_ap(d, d, d, 8, d, 1, 1, 0, None, d, 8, d) == _lib.Y3_EINVAL
    assert b'y3_voc_ap' in L.y3_last_error()


def test_reference_vectors(emul):
    case, results = vc.golden()
    assert len(case.preds) == 70 and sum(len(v) for v in case.gt_dict.values()) == 45 and len(case.image_ids) == 12
    vc.assert_distinct_scores(case)
    for m07 in (False, True):
        want = np.array([r[2:] for r in results if bool(r[1]) == m07], np.float64)
        assert want.shape == (6, 5)
        got, _, _ = emulate(emul, case, 0.5, m07)
        vc.assert_table(got, want, m07, 'golden m07=%d' % m07)
        assert got[5].tolist() == [1e-6, 1e-6, 0., 0., 0.]          # the class with neither detection nor object
        np.testing.assert_array_equal(vc.reference_table(case, 0.5, m07), want)      # (the host path, for the record)


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('fp32', [True, False])
def test_random_sets_against_voc_eval(emul, seed, fp32):
    case = vc.random_case(seed, fp32=fp32)
    vc.assert_distinct_scores(case)
    assert 400 <= len(case.preds) <= 900
    for thres in (0.5, 0.3):
        for m07 in (False, True):
            got, _, _ = emulate(emul, case, thres, m07)
            vc.assert_table(got, vc.reference_table(case, thres, m07), m07, 'seed %d thres %g m07=%d' % (seed, thres, m07))
    assert (got[:, 2] > 0.2).all() and (got[:, 3] < 0.9).all()      # a set with both true and false positives in every class


@pytest.mark.parametrize('name', sorted(vc.corner_cases()))
def test_corner_cases(emul, name):
    case, (cls, flags) = vc.corner_cases()[name]
    vc.assert_distinct_scores(case)
    for m07 in (False, True):
        got, order, tp = emulate(emul, case, 0.5, m07)
        vc.assert_table(got, vc.reference_table(case, 0.5, m07), m07, name)
    ranked_labels = np.array([case.preds[k][6] for k in order])
    assert tp[ranked_labels == cls].tolist() == flags
    if name == 'iou_exactly_half':
        from yolov3_tensorflow_amd.utils.eval_utils import voc_eval
        assert got[0, :4].tolist() == [1., 1., 0., 0.]
        got, _, tp = emulate(emul, case, np.nextafter(0.5, 0.), False)      # ... and a true positive just under it
        assert tp.tolist() == [1]
    if name == 'npos_zero':
        assert np.isnan(got[1, 2]) and got[1, 3] == 0. and got[2].tolist() == [1e-6, 1e-6, 0., 0., 0.]
        assert np.isnan(emulate(emul, case, 0.5, False)[0][1, 4]) and got[1, 4] == 0.      # area AP NaN; 11 points 0, like numpy


def test_tied_scores_rank_by_arrival(emul):
    case = vc.tied_case()
    scores = [p[5] for p in case.preds if p[6] == 0]
    assert len(set(scores)) <= 8 < len(scores)
    for m07 in (False, True):
        got, order, _ = emulate(emul, case, 0.5, m07)
        vc.assert_table(got, vc.reference_table(case, 0.5, m07, fn=vc.voc_eval_stable), m07, 'tied m07=%d' % m07)
    key = [(case.preds[k][6], -case.preds[k][5], k) for k in order]
    assert key == sorted(key)
    # the restatement is voc_eval where voc_eval's order is defined
    distinct = vc.random_case(2)
    np.testing.assert_array_equal(vc.reference_table(distinct, 0.5, False, fn=vc.voc_eval_stable), vc.reference_table(distinct, 0.5, False))
