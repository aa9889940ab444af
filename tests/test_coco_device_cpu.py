"""CPU tests of COCO evaluation: eval_utils.coco_eval against hand-worked values and against voc_eval where the two rules
coincide, and the device evaluator's arithmetic (include/yolo355.h: y3_coco_match / y3_coco_ap / y3_coco_summary) - the
per-element functions the kernels are made of (csrc/y3_coco_px.h) run on the host (tests/coco_emul.cpp) against coco_eval on the
pins, seeded random sets and the corner cases of the rule.  tests/test_coco_device_gpu.py repeats the comparison with the
kernels themselves."""
import contextlib
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import coco_cases as cc


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('coco_emul') / 'libcoco_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math',
                           os.path.join(ROOT, 'tests', 'coco_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3c_emulate.restype = ctypes.c_int
    lib.y3c_emulate.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 11
    return lib


def emulate(emul, case):
    from yolov3_tensorflow_amd.utils import eval_utils
    a = cc.arena_of(case)
    rows, K = len(case.preds), case.class_num
    out = {'precision': np.full((10, 101, K, 4, 3), -7.), 'recall': np.full((10, K, 4, 3), -7.), 'per_class': np.full((K, 12), -7.),
           'stats': np.full(12, -7.)}
    order, matched, ignored = np.full(rows, -1, np.int32), np.zeros(rows, np.uint64), np.zeros(rows, np.uint64)
    grank, npig = np.zeros(rows, np.uint8), np.zeros((K, 4), np.int32)
    p = lambda x: None if x is None else x.ctypes.data
    assert emul.y3c_emulate(p(a['box']), p(a['score']), p(a['label']), p(a['image']), rows, p(a['gt_start']), p(a['gt_box']),
                            p(a['gt_label']), p(a['area_scale']), a['num_images'], a['num_gt'], K, p(eval_utils.COCO_IOU_THRS),
                            p(eval_utils.COCO_REC_THRS), p(out['precision']), p(out['recall']), p(out['per_class']), p(out['stats']),
                            p(order), p(matched), p(ignored), p(grank), p(npig)) == 0
    out.update(order=order, matched=matched, ignored=ignored, group_rank=grank, npig=npig)
    return out


def test_the_device_interface_exists():
    """The C entries, their prototypes, the build entry, coco_eval and DeviceEval.finish_coco (this is what fails on a tree
    without the feature)."""
    from yolov3_tensorflow_amd import _lib, build
    from yolov3_tensorflow_amd.utils import eval_utils
    for name in ('y3_coco_match', 'y3_coco_ap', 'y3_coco_summary', 'y3_coco_match_scratch_bytes', 'y3_coco_ap_scratch_bytes',
                 'y3_coco_ap_pass', 'y3_coco_lds_objects'):
        assert name in _lib.PROTOTYPES
    assert ('y3_coco.hip', ['-ffp-contract=off']) in build.SOURCES
    assert callable(eval_utils.coco_eval) and callable(eval_utils.parse_gt_area_scale)
    assert callable(eval_utils.DeviceEval.finish_coco)
    assert eval_utils.COCO_IOU_THRS[8] == 0.8999999999999999 and eval_utils.COCO_IOU_THRS[0] == 0.5 and eval_utils.COCO_IOU_THRS[5] == 0.75


def test_host_entry_points_validate_before_launching():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert L.y3_abi_version() == 5
    assert L.y3_coco_ap_pass() >= 256 and L.y3_coco_ap_pass() % 64 == 0 and L.y3_coco_lds_objects() >= 64
    assert L.y3_coco_match_scratch_bytes(0, 5) == 0 and L.y3_coco_match_scratch_bytes(5, -1) == 0 and L.y3_coco_ap_scratch_bytes(0) == 0
    assert L.y3_coco_match_scratch_bytes(1000, 45) >= 45 * 8 and L.y3_coco_ap_scratch_bytes(1000) >= 1000 * 21
    assert L.y3_coco_match_scratch_bytes(1000, 45) == 512 and L.y3_coco_ap_scratch_bytes(1000) == 21504
    assert L.y3_coco_match_scratch_bytes(7, 0) == 256
    d = ctypes.c_void_p(4096)
    thr = (ctypes.c_double * 101)(*np.linspace(0., 1., 101))
    big = 1 << 30
    match = lambda *a: L.y3_coco_match(*a)
    ok = [d, d, d, d, d, 8, None, d, d, d, None, 1, 1, 1, thr, d, big, d, d, d, d]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    assert match(*with_(0, None)) == _lib.Y3_EINVAL                    # no context
    assert match(*with_(14, None)) == _lib.Y3_EINVAL                   # no thresholds
    assert match(*with_(20, None)) == _lib.Y3_EINVAL                   # no npig
    assert match(*with_(5, 0)) == _lib.Y3_EINVAL                       # rows
    assert match(*with_(11, 0)) == _lib.Y3_EINVAL                      # num_images
    assert match(*with_(13, 0)) == _lib.Y3_EINVAL                      # class_num
    assert match(*with_(16, 0)) == _lib.Y3_EINVAL                      # scratch too small
    assert match(*with_(15, ctypes.c_void_p(4100))) == _lib.Y3_EINVAL      # misaligned scratch
    a = with_(11, 1 << 20)
    a[13] = 1 << 20
    assert match(*a) == _lib.Y3_EINVAL                                 # num_images * class_num beyond 2^31 - 1
    assert b'y3_coco_match' in L.y3_last_error()
    ap_ok = [d, d, d, d, d, d, d, 8, None, d, 1, thr, d, big, d, d]

    def ap_with(i, v):
        a = list(ap_ok)
        a[i] = v
        return a
    assert L.y3_coco_ap(*ap_with(11, None)) == _lib.Y3_EINVAL          # no recall thresholds
    assert L.y3_coco_ap(*ap_with(7, 0)) == _lib.Y3_EINVAL              # rows
    assert L.y3_coco_ap(*ap_with(10, 0)) == _lib.Y3_EINVAL             # class_num
    assert L.y3_coco_ap(*ap_with(10, 200000)) == _lib.Y3_EINVAL        # 12120 * class_num beyond 2^31 - 1
    assert L.y3_coco_ap(*ap_with(13, 100)) == _lib.Y3_EINVAL           # scratch too small
    assert L.y3_coco_ap(*ap_with(14, None)) == _lib.Y3_EINVAL          # no output
    assert b'y3_coco_ap' in L.y3_last_error()
    assert L.y3_coco_summary(d, d, d, 0, d, d) == _lib.Y3_EINVAL
    assert L.y3_coco_summary(d, d, None, 1, d, d) == _lib.Y3_EINVAL
    assert L.y3_coco_summary(d, d, d, 200000, d, d) == _lib.Y3_EINVAL
    assert b'y3_coco_summary' in L.y3_last_error()


@pytest.mark.parametrize('name', sorted(cc.pins()))
def test_hand_worked_pins(name):
    """coco_eval against values derived from the rule by hand; 1 / (1 + eps) is 0.9999999999999998, not 1.0."""
    case, expect = cc.pins()[name]
    got = cc.reference(case)
    assert cc.ONE == 0.9999999999999998 and 1. / (2. + cc.EPS) == 0.5 and 2. / (2. + cc.EPS) == 1.0
    print(name, got['stats'].tolist(), expect)
    for g, w in zip(got['stats'], expect):
        assert g == w if w == -1 else abs(g - w) <= 1010 * 2.0 ** -52      # (a mean over at most 1,010 entries)
    np.testing.assert_array_equal(got['per_class'][0], got['stats'])
    p = got['precision']
    if name in 'AD':
        assert (p[:, :, 0, 0, 2] == cc.ONE).all() and (p[:, :, 0, 1, 2] == cc.ONE).all() and (p[:, :, 0, 3, :] == -1).all()
        assert ((p[:, :, 0, 2, 2] == cc.ONE).all() if name == 'D' else (p[:, :, 0, 2, :] == -1).all())
    if name == 'B':
        assert (p[0, :, 0, 0, 2] == cc.ONE).all() and (p[1:, :, 0, 0, 2] == 0).all()
    if name == 'C':
        assert (p[:, :51, 0, 0, 2] == 0.5).all() and (p[:, 51:, 0, 0, 2] == 0).all() and (p[:, :, 0, 0, 0] == 0).all()
    if name == 'E':
        assert (p[:, :, 0, 0, 2] == 1.0).all() and (p[:, :51, 0, 0, 0] == cc.ONE).all() and (p[:, 51:, 0, 0, 0] == 0).all()


def test_recall_at_half_is_voc_evals_where_the_rules_coincide():
    from yolov3_tensorflow_amd.utils.eval_utils import voc_eval
    case, ious = cc.voc_comparable_case()
    assert len(case.preds) > 60
    hits = 0
    for d in case.preds:
        over = [o for o in case.gt_dict[d[0]] if o[4] == d[6] and max(ious(d, o)) > 0.]
        assert len(over) <= 1                                                   # at most one object of its class
        for o in case.gt_dict[d[0]]:
            assert all(not 0.45 <= v <= 0.55 for v in ious(d, o))               # in the plain and in the +1 form
        hits += bool(over) and min(ious(d, over[0])) > 0.55
    assert hits > 20
    got = cc.reference(case)
    for k in range(case.class_num):
        with contextlib.redirect_stdout(io.StringIO()):
            npos, nd, rec, _, _ = voc_eval(case.gt_dict, case.preds, k, iou_thres=0.5)
        assert npos >= 1 and nd >= 1 and 0 < rec
        assert got['recall'][0, k, 0, 2] == rec


def test_area_scale_of_an_annotation_file(tmp_path):
    from yolov3_tensorflow_amd.utils import eval_utils
    ann = tmp_path / 'val.txt'
    ann.write_text('0 a.jpg 200 100 1 10 10 50 50\n1 b.jpg 100 400 0 1 2 30 40 2 5 5 9 9\n')
    boxed = eval_utils.parse_gt_area_scale(str(ann), [100, 100], True)
    plain = eval_utils.parse_gt_area_scale(str(ann), [100, 100], False)
    assert boxed == {0: 1. / (0.5 * 0.5), 1: 1. / (0.25 * 0.25)} and plain == {0: 1. / (0.5 * 1.0), 1: 1. / (1.0 * 0.25)}
    eval_utils.gt_dict = {}
    gt = eval_utils.parse_gt_rec(str(ann), [100, 100], False)
    eval_utils.gt_dict = {}
    x0, y0, x1, y1 = gt[0][0][:4]
    assert (x1 - x0) * (y1 - y0) * plain[0] == 40. * 40.                        # back in original pixels


@pytest.mark.parametrize('name', sorted(cc.corner_cases()))
def test_corner_cases(emul, name):
    case = cc.corner_cases()[name]
    want, got = cc.reference(case), emulate(emul, case)
    cc.assert_result(got, want, name)
    r, p = want['recall'], want['precision']
    if name == 'iou_exactly_threshold':      # the IoU 1/2 object is found at t = 0.5 only, the IoU 3/4 one up to t = 0.75
        assert r[:, 0, 0, 2].tolist() == [1., .5, .5, .5, .5, .5, 0., 0., 0., 0.]
    if name == 'equal_ious_later_wins':
        assert r[:4, 0, 0, 2].tolist() == [1., 1., 1., 1.] and r[4:, 0, 0, 2].tolist() == [.5] * 6
    if name == 'non_ignored_before_better_ignored':
        bit = lambda word, t, a: int(word) >> (t * 4 + a) & 1
        assert [bit(got['matched'][0], t, 1) for t in range(10)] == [1] * 9 + [0]          # 0.909 < 0.95
        assert [bit(got['ignored'][0], t, 1) for t in range(10)] == [0] * 6 + [1] * 4      # the ignored object above 0.75
        assert r[:, 0, 1, 2].tolist() == [1.] * 6 + [0.] * 4 and r[:, 0, 0, 2].tolist() == [.5] * 9 + [0.]
    if name == 'areas_on_the_boundaries':
        assert got['npig'].tolist() == [[2, 1, 2, 1]] and (r[:, 0, :, 2] == 1.).all()
    if name == 'area_scale_moves_an_object':
        assert got['npig'].tolist() == [[2, 1, 1, 0]]
    if name == 'empty_classes_and_images':
        assert (p[:, :, 1, :2] == 0).all() and (r[:, 1, :2] == 0).all() and (p[:, :, 1, 2:] == -1).all()      # (its object is small)
        assert (p[:, :, 2:] == -1).all() and (r[:, 2:] == -1).all()
        assert want['per_class'][1].tolist() == [0.] * 4 + [-1.] * 2 + [0.] * 4 + [-1.] * 2 and (want['per_class'][2:] == -1).all()
    if name == 'tied_scores':
        rows = [case.preds[k] for k in got['order']]
        assert [(x[0], x[1]) for x in rows] == [(1, 0.), (2, 50.), (2, 0.), (3, 20.), (3, 100.), (3, 0.)]
    if name == 'more_than_100_detections':
        ranks = got['group_rank'][[case.preds[k][0] == 1 for k in got['order']]]
        assert ranks.tolist() == list(range(255)) + [255] * 5
        assert not got['matched'][got['group_rank'] >= 100].any() and r[0, 0, 0, 2] == 3. / 4 and got['matched'][:100].any()
    if name == 'seventy_objects_in_one_group':
        assert got['npig'][0, 0] == 70 and 0.5 < r[0, 0, 0, 2] < 1.


@pytest.mark.parametrize('seed,images,classes', [(1, 12, 4), (2, 40, 5), (3, 6, 3)])
@pytest.mark.parametrize('fp32', [True, False])
def test_random_sets_against_coco_eval(emul, seed, images, classes, fp32):
    case = cc.random_case(seed, images, classes, fp32=fp32)
    assert 60 <= len(case.preds) <= 900
    want = cc.reference(case)
    cc.assert_result(emulate(emul, case), want, 'seed %d' % seed)
    assert (want['stats'] > 0).all() and (want['stats'] < 1).all()      # true and false positives in every size and at every cut
    scales = {k: 0.4 + 0.35 * i for i, k in enumerate(case.image_ids)}
    scaled = case._replace(area_scale=scales)
    cc.assert_result(emulate(emul, scaled), cc.reference(scaled), 'seed %d scaled' % seed)


def test_more_objects_than_the_lds_words_and_a_list_longer_than_two_passes(emul):
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    case = cc.many_objects_case(L.y3_coco_lds_objects() + 8)
    want = cc.reference(case)
    cc.assert_result(emulate(emul, case), want, 'many objects')
    assert 0.02 < want['stats'][0] < 0.2 and want['stats'][8] < 0.1      # (40 of the objects have a detection)
    case = cc.long_case(L.y3_coco_ap_pass())
    want = cc.reference(case)
    cc.assert_result(emulate(emul, case), want, 'long')
    assert 0.02 < want['stats'][0] < 0.9


def test_report_lines():
    from yolov3_tensorflow_amd.utils.eval_utils import coco_summary_lines
    lines = coco_summary_lines(np.arange(12) / 16.)
    assert lines[0] == 'Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.000'
    assert lines[7] == 'Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 0.438'
    assert len(lines) == 12 and lines[11].endswith('area= large | maxDets=100 ] = 0.688')


def test_both_scripts_take_the_flag_and_default_to_off():
    import sys
    sys.path.insert(0, ROOT)
    import eval as eval_script
    import train as train_script
    assert eval_script.OPTIONS[-1][0] == 'coco_metric' and eval_script.OPTIONS[-1][2] is False      # a new trailing row
    for script in (eval_script, train_script):
        parser = script.build_parser()
        assert parser.parse_args([]).coco_metric is False
        assert parser.parse_args(['--coco_metric', 'true']).coco_metric is True
