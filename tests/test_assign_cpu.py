"""Multi-anchor positives, the ignore threshold and the IoU objectness target without a GPU: the host form of the assignment
rule (utils.data_utils.process_box_host) against the reference's goldens at its default and against records worked by hand at
darknet's 0.213; the fp64 oracle of tests/assign_cases.py against oracle.train_ref at (0.5, 0), against hand values, and in
fp32 against itself in fp64 under the gates the GPU tests use; the conditioning of the cases; the Python surface."""
import math

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
import assign_cases as AC
import iou_loss_cases as IC
import test_loss_gpu as TL


# ---- the assignment rule --------------------------------------------------------------------------------------------------
def test_process_box_host_at_the_default_is_the_reference_bit_for_bit(golden):
    for thresh in (1.0, 2.0):
        for i in range(int(golden['process_box_n'])):
            boxes, labels = golden['process_box_%d_boxes' % i], golden['process_box_%d_labels' % i]
            ys = AC.host(boxes, labels, [416, 416], 80, thresh)
            for y, k in zip(ys, ('y13', 'y26', 'y52')):
                want = golden['process_box_%d_%s' % (i, k)]
                assert y.dtype == np.float32 and y.shape == want.shape
                np.testing.assert_array_equal(y, want)
    from yolov3_tensorflow_amd.utils import data_utils
    boxes, labels = golden['process_box_0_boxes'], golden['process_box_0_labels']
    for y, k in zip(data_utils.process_box_host(boxes, labels, [416, 416], 80, COCO_ANCHORS), ('y13', 'y26', 'y52')):
        np.testing.assert_array_equal(y, golden['process_box_0_%s' % k])


@pytest.mark.parametrize('size', [(40, 50), (12, 14), (300, 280)])
def test_process_box_host_at_darknet_threshold_by_hand(size):
    """exactly the records of the best anchor and of the extras, each in the cell of the centre at its own stride, and no
    others; at the default only the best anchor's"""
    best, extras = AC.HAND[size]
    cx, cy, label, mix = 203., 117., 1, 0.625
    b = np.array([AC.box(cx, cy, size[0], size[1], mix)], np.float32)
    got = AC.records(AC.host(b, [label], [416, 416], 3, AC.DARKNET_THRESH))
    assert got == AC.expected_records(cx, cy, size[0], size[1], {best} | extras, [label], mix)
    assert {(k, gx, gy) for k, gx, gy in got} == {(k, 203 // AC.STRIDE_OF(k), 117 // AC.STRIDE_OF(k)) for k in {best} | extras}
    assert AC.records(AC.host(b, [label], [416, 416], 3, 1.0)) == AC.expected_records(cx, cy, size[0], size[1], {best}, [label], mix)


def test_a_later_box_overwrites_the_shared_record_and_keeps_both_class_bits():
    boxes, labels, cell = AC.collision_case()
    got = AC.records(AC.host(boxes, labels, [416, 416], 3, AC.DARKNET_THRESH))
    first = AC.expected_records(200., 180., 40, 50, {3} | AC.HAND[(40, 50)][1], [0], 0.5)
    second = AC.expected_records(200., 180., 60, 80, {5} | AC.HAND[(60, 80)][1], [2], 0.25)
    assert set(first) & set(second) == {cell, (4, 12, 11), (5, 12, 11)}      # anchors 3, 4, 5: all of the 26-grid's
    want = dict(first)
    want.update(second)                                   # the second box's geometry and mix weight wherever both wrote ...
    for k in set(first) & set(second):
        want[k] = (second[k][0], [0, 2], second[k][2])    # ... and both class bits
    assert got == want
    assert got[cell][0] == (200., 180., 60., 80.) and got[cell][1] == [0, 2]
    # in the other order the first box's geometry wins, with the same bits
    swapped = AC.records(AC.host(boxes[::-1], labels[::-1], [416, 416], 3, AC.DARKNET_THRESH))
    assert swapped[cell][0] == (200., 180., 40., 50.) and swapped[cell][1] == [0, 2]


def test_process_box_host_skips_what_the_kernel_skips_and_refuses_bad_thresholds():
    boxes, labels, counts = AC.gpu_case()
    ys = AC.host_batch(boxes, labels, counts, [AC.GPU_W, AC.GPU_H], AC.GPU_C, AC.DARKNET_THRESH)
    assert [y.shape for y in ys] == [(3, 2, 3, 3, 9), (3, 4, 6, 3, 9), (3, 8, 12, 3, 9)]
    assert all((y[1][..., :-1] == 0).all() and (y[1][..., -1] == 1).all() for y in ys)          # counts[1] == 0
    rec0, rec2 = AC.records([y[0] for y in ys]), AC.records([y[2] for y in ys])
    assert any(bits == [] for _, bits, _ in rec0.values())            # the label outside [0, C) sets no bit
    assert (3, 3, 2) in rec0 and rec0[(3, 3, 2)][1] == [0, 2]         # the collision pair at (60, 44): 26-grid cell (3, 2)
    # image 2: the centre at cx = -4 writes nothing; label -1 sets no bit; the last cell is written; rows past the count are not read
    assert all(geo[0] in (40., 95.5) for geo, _, _ in rec2.values()) and {geo[0] for geo, _, _ in rec2.values()} == {40., 95.5}
    assert (0, 11, 7) in rec2 and all(bits in ([], [2]) for _, bits, _ in rec2.values())
    from yolov3_tensorflow_amd.utils import data_utils
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            data_utils.process_box_host(boxes[0], labels[0], [96, 64], 3, COCO_ANCHORS, bad)


# ---- the conf rule's oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(TL.CASES))
def test_oracle_at_the_defaults_is_train_ref_exactly(case):
    fm, y = TL.inputs(case)
    for smooth, focal in ((False, False), (True, True)):
        want4, wantg = TL.reference(case, smooth, focal)
        got4, gotg = AC.evaluate(case, 'mse', smooth, focal, 0.5, 0.0, data=(fm, y))
        assert got4 == want4
        np.testing.assert_array_equal(gotg, wantg)


def test_oracle_with_an_iou_kind_at_the_defaults_is_the_iou_oracle_exactly():
    for case in ('5x7_c20', '1x2_c1'):
        want4, wantg = IC.reference(case, 'ciou', True, True)
        got4, gotg = AC.evaluate(case, 'ciou', True, True, 0.5, 0.0, data=IC.inputs(case))
        assert got4 == want4
        np.testing.assert_array_equal(gotg, wantg)


def _one_record(f, true_box, ratio, thresh=0.5, focal=False):
    """a 1 x 1 grid on a 32 x 32 image, one class: record (anchor 0) holds `true_box`, logits f [3][6]; returns (z, conf)"""
    y = np.zeros((1, 1, 1, 3, 7), np.float32)
    y[..., -1] = 1.
    y[0, 0, 0, 0] = list(true_box) + [1., 1., 1.]
    g = AC.graph_for(1, [32, 32])
    fm = torch.tensor(np.asarray(f, np.float64).reshape(1, 1, 1, 18))
    yt = torch.tensor(y, dtype=torch.float64)
    z = AC.objectness_target(g.reorg(fm, COCO_ANCHORS[6:9])[1], yt, ratio)
    parts = g.loss_layer(fm, y, COCO_ANCHORS[6:9], False, focal, 'mse', thresh, ratio)
    return z.reshape(3).numpy(), float(parts[2])


def _bce(z, x):
    return max(x, 0.) - x * z + math.log1p(math.exp(-abs(x)))


def test_objectness_target_by_hand():
    aw, ah = float(COCO_ANCHORS[6][0]), float(COCO_ANCHORS[6][1])
    logit = lambda p: math.log(p / (1 - p))
    x = [0.7, -1.1, 0.4]
    f = np.zeros((3, 6))
    f[:, 4] = x
    f[1:, 0:2] = 3.                         # the two records without an object: far from the true box, tiny
    f[1:, 2:4] = -6.
    # the prediction IS the true box (16, 12, 8, 6): IoU 1 up to the union's 1e-10
    f[0, 0:4] = [logit(16 / 32.), logit(12 / 32.), math.log(8 / aw), math.log(6 / ah)]
    z, conf = _one_record(f, (16., 12., 8., 6.), 1.0)
    assert z[1] == 0 and z[2] == 0 and 0 <= 1 - z[0] < 1e-10
    assert abs(conf - (_bce(z[0], x[0]) + _bce(0, x[1]) + _bce(0, x[2]))) < 1e-12
    z0, conf0 = _one_record(f, (16., 12., 8., 6.), 0.0)
    assert z0.tolist() == [1., 0., 0.] and abs(conf0 - (_bce(1, x[0]) + _bce(0, x[1]) + _bce(0, x[2]))) < 1e-12
    # disjoint: the true box (4, 4, 4, 4), the prediction at (28, 28) and 2 px wide: target 0, the conf term is bce(0, x)
    f[0, 0:4] = [logit(28 / 32.), logit(28 / 32.), math.log(2 / aw), math.log(2 / ah)]
    z, conf = _one_record(f, (4., 4., 4., 4.), 1.0)
    assert z.tolist() == [0., 0., 0.]
    assert abs(conf - sum(_bce(0, v) for v in x)) < 1e-12
    # IoU 0.5 (the same centre and height, half the width) with r = 0.5: target 0.75
    f[0, 0:4] = [logit(16 / 32.), logit(12 / 32.), math.log(4 / aw), math.log(6 / ah)]
    z, conf = _one_record(f, (16., 12., 8., 6.), 0.5)
    assert abs(z[0] - 0.75) < 1e-10
    # ... under focal the factor is (z - p)^2
    _, conf_f = _one_record(f, (16., 12., 8., 6.), 0.5, focal=True)
    sig = lambda v: 1 / (1 + math.exp(-v))
    want = _bce(z[0], x[0]) * (z[0] - sig(x[0])) ** 2 + sum(_bce(0, v) * sig(v) ** 2 for v in x[1:])
    assert abs(conf_f - want) < 1e-12
    # a prediction that is inf wide (inf / inf): counted as 0, nothing non-finite
    pred = torch.tensor([[16., 12., float('inf'), float('inf')]], dtype=torch.float32)
    yt = torch.tensor([[16., 12., 8., 6., 1., 1., 1.]], dtype=torch.float32)
    assert AC.objectness_target(pred, yt, 1.0).tolist() == [[0.]]


def test_the_ignore_threshold_moves_records_in_and_out_of_the_conf_term():
    """0.7 ignores more records than 0.5 than 0.3 (cmask is monotone), and the conf term differs between them"""
    case = 'many_boxes'
    fm, y = AC.inputs(case)
    best = TL.best_iou64(case, fm, y)
    non = y[..., 4] == 0
    counts = [int(((best < t) & non).sum()) for t in AC.THRESHOLDS]
    assert counts[0] < counts[1] < counts[2]
    conf = [AC.reference(case, 'mse', False, False, t, 0.0)[0][2] for t in AC.THRESHOLDS]
    assert conf[0] < conf[1] < conf[2]


@pytest.mark.parametrize('case', AC.CASE_NAMES)
def test_cases_are_conditioned_for_every_threshold(case):
    """inputs() asserts the margin on every record (and, for many_boxes, more than 100 records on either side of each
    threshold); here: again from the cached arrays, and the cases still hold what iou_loss_cases put there"""
    fm, y = AC.inputs(case)
    best = TL.best_iou64(case, fm, y)
    for t in AC.THRESHOLDS:
        assert not (np.abs(best - t) < TL.IOU_MARGIN).any()
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    f = fm.reshape(n, gh, gw, 3, 5 + C)
    m = y[..., 4] != 0
    assert int((((f[..., 2] == 90.) | (f[..., 3] == -90.)) & ~m).sum()) == 2
    if case == '5x7_c20':
        assert int((((f[..., 2] == 25.) | (f[..., 3] == -25.)) & m).sum()) >= 2
    assert fm is AC.inputs(case)[0]


@pytest.mark.parametrize('case', AC.CASE_NAMES)
def test_the_gates_are_reachable_in_fp32(case):
    """the oracle in fp32 against itself in fp64 on the GPU tests' cases and rules, under their gates"""
    for kind in ('mse', 'ciou'):
        for (thresh, ratio), (smooth, focal) in zip(AC.RULES, ((False, False), (True, True), (True, True))):
            want4, wantg = AC.reference(case, kind, smooth, focal, thresh, ratio)
            got4, gotg = AC.evaluate(case, kind, smooth, focal, thresh, ratio, dtype=torch.float32)
            assert np.isfinite(gotg).all() and np.isfinite(got4).all()
            AC.check_gates(got4, gotg, want4, wantg, 'fp32 oracle %s %s t=%g r=%g' % (case, kind, thresh, ratio))


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_model_setters_reject_bad_values():
    import yolov3_tensorflow_amd as y3
    model = y3.yolov3(3, COCO_ANCHORS)
    assert (model.ignore_thresh, model.obj_iou_ratio) == (0.5, 0.0)
    model.ignore_thresh, model.obj_iou_ratio = 0.7, 1
    assert (model.ignore_thresh, model.obj_iou_ratio) == (0.7, 1.0)
    model.ignore_thresh, model.obj_iou_ratio = 0, 0
    for name in ('ignore_thresh', 'obj_iou_ratio'):
        for bad in (-0.01, 1.01, float('nan'), float('inf')):
            with pytest.raises(ValueError):
                setattr(model, name, bad)
        assert getattr(model, name) == 0.0
        with pytest.raises((TypeError, ValueError)):
            setattr(model, name, 'high')


def test_feeder_and_process_box_refuse_bad_thresholds_before_any_device_work():
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils import data_utils
    for bad in (0.0, -0.5, float('nan')):
        with pytest.raises(ValueError):
            Feeder(['0 a.jpg 10 10 0 1 1 5 5'], 1, 3, [96, 64], COCO_ANCHORS, mode='val', backend='thread', pixels='host',
                   assign_iou_thresh=bad)
        with pytest.raises(ValueError):
            data_utils.process_box_batch(np.zeros((1, 1, 5), np.float32), [[0]], [1], [96, 64], 3, COCO_ANCHORS, bad)
    f = Feeder(['0 a.jpg 10 10 0 1 1 5 5'], 1, 3, [96, 64], COCO_ANCHORS, mode='val', backend='thread', pixels='host')
    assert f.assign_iou_thresh == 1.0
    assert Feeder(['0 a.jpg 10 10 0 1 1 5 5'], 1, 3, [96, 64], COCO_ANCHORS, mode='val', backend='thread', pixels='host',
                  assign_iou_thresh=0.213).assign_iou_thresh == 0.213


def test_script_options_parse():
    import importlib
    import os
    import sys
    from conftest import ROOT
    import train
    p = train.build_parser()
    a = p.parse_args([])
    assert (a.ignore_thresh, a.obj_iou_ratio, a.assign_iou_thresh) == (0.5, 0.0, 1.0)
    a = p.parse_args(['--ignore_thresh', '0.7', '--obj_iou_ratio', '1', '--assign_iou_thresh', '0.213'])
    assert (a.ignore_thresh, a.obj_iou_ratio, a.assign_iou_thresh) == (0.7, 1.0, 0.213)
    assert '0.213' in p.format_help()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        tb = importlib.import_module('train_bench')
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    a = tb.build_parser().parse_args([])
    assert (a.ignore_thresh, a.obj_iou_ratio) == (0.5, 0.0)
    a = tb.build_parser().parse_args(['--ignore_thresh', '0.7', '--obj_iou_ratio', '1'])
    assert (a.ignore_thresh, a.obj_iou_ratio) == (0.7, 1.0)
