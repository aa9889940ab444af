"""The IoU box losses without a GPU: the fp64 oracle of tests/iou_loss_cases.py against values worked by hand, the oracle in
fp32 against itself in fp64 on the cases the GPU tests run (what fp32 arithmetic alone costs under the project's loss gates:
each term within 1e-4 |ref| + 1e-6, the gradient within 2e-4 of its max magnitude), the case census, and the Python surface
(yolov3.box_loss, train.py --box_loss, tools/train_bench.py --box_loss)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, COCO_ANCHORS
import iou_loss_cases as IC
import test_loss_gpu as TL


def _x(kind, p, t):
    return float(IC.box_x(kind, torch.tensor([p], dtype=torch.float64), torch.tensor([t], dtype=torch.float64))[0])


@pytest.mark.parametrize('kind', sorted(IC.KINDS))
def test_identical_boxes_give_a_term_of_zero(kind):
    box = [40., 30., 10., 20.]
    assert abs(1. - _x(kind, box, box)) < 1e-11          # (the 1e-10 of the union over an area of 200)
    y = torch.zeros(1, 1, 1, 3, 7, dtype=torch.float64)
    y[0, 0, 0, 1] = torch.tensor(box + [1., 1., 0.5])
    pred = torch.zeros(1, 1, 1, 3, 4, dtype=torch.float64)
    pred[..., 2:] = 1.                                   # the two records without an object: any box
    pred[0, 0, 0, 1] = torch.tensor(box)
    assert abs(float(IC.box_term(kind, pred, y, (100, 100), 1))) < 1e-11


def test_two_disjoint_unit_squares_three_apart():
    """inter 0, union 2, enclosing box 4 x 1: GIoU = 0 - (4 - 2) / 4, DIoU = 0 - 3^2 / (4^2 + 1^2); CIoU = DIoU (equal shapes)"""
    p, t = [0., 0., 1., 1.], [3., 0., 1., 1.]
    assert abs(_x('giou', p, t) - (-0.5)) < 1e-10
    assert abs(_x('diou', p, t) - (-9. / 17.)) < 1e-10
    assert abs(_x('ciou', p, t) - (-9. / 17.)) < 1e-10
    # the weight: one object record, mix-up weight 0.5, a 10 x 10 image, batch of 2
    y = torch.zeros(1, 1, 1, 3, 7, dtype=torch.float64)
    y[0, 0, 0, 0] = torch.tensor(t + [1., 1., 0.5])
    pred = torch.ones(1, 1, 1, 3, 4, dtype=torch.float64)
    pred[0, 0, 0, 0] = torch.tensor(p)
    want = (1. + 0.5) * (2. - 0.1 * 0.1) * 0.5 / 2
    assert abs(float(IC.box_term('giou', pred, y, (10, 10), 2)) - want) < 1e-10


def test_a_square_against_a_two_to_one_rectangle_of_equal_centre():
    """square 2 x 2 inside the rectangle 4 x 2: iou 4 / 8, no centre distance, atan(2) - atan(1) = atan(1 / 3):
    v = (4 / pi^2) atan(1/3)^2, alpha = v / (1/2 + v), CIoU = 1/2 - alpha v"""
    p, t = [5., 5., 2., 2.], [5., 5., 4., 2.]
    v = 4. / math.pi ** 2 * math.atan(1. / 3.) ** 2
    alpha = v / (0.5 + v)
    assert abs(_x('diou', p, t) - 0.5) < 1e-10
    assert abs(_x('giou', p, t) - 0.5) < 1e-10           # the enclosing box is the rectangle: no penalty
    assert abs(_x('ciou', p, t) - (0.5 - alpha * v)) < 1e-10
    # alpha is a constant of the gradient: d CIoU / d pw holds -alpha dv/dpw and no d alpha term
    pt = torch.tensor([p], dtype=torch.float64, requires_grad=True)
    IC.box_x('ciou', pt, torch.tensor([t], dtype=torch.float64)).sum().backward()
    dv_dpw = 2 * (4. / math.pi ** 2) * math.atan(1. / 3.) * (-1.) * (2. / (2. ** 2 + 2. ** 2))
    # (d iou / d pw: inter = pw * 2, union = 8: 2 / 8)
    assert abs(float(pt.grad[0, 2]) - (0.25 - alpha * dv_dpw)) < 1e-10


def test_the_case_set_holds_what_the_gpu_tests_are_about():
    census = IC.build()
    print(census)
    assert census['disjoint'] >= 1 and census['pred_encloses_true'] >= 1 and census['saturated'] >= 2
    assert census['overflow_non_object'] == 2 * len(IC.CASE_NAMES)
    for case in IC.CASE_NAMES:                           # test_loss_gpu.py's cached inputs are untouched
        fm0, _ = TL.inputs(case)
        assert not (np.abs(fm0) == 90.).any()


@pytest.mark.parametrize('kind', sorted(IC.KINDS))
@pytest.mark.parametrize('case', IC.CASE_NAMES)
def test_fp32_evaluation_of_the_oracle_is_inside_the_gates(case, kind):
    """Worst figures (printed): see the table in test_iou_loss_gpu.py's docstring."""
    for smooth, focal in IC.MODES:
        want4, wantg = IC.reference(case, kind, smooth, focal)
        got4, gotg = IC.evaluate(case, kind, smooth, focal, torch.float32)
        assert np.isfinite(gotg).all() and np.isfinite(got4).all()
        err = TL.rel_err(gotg.astype(np.float64), wantg)
        print('%s %s smooth=%d focal=%d: fp32 box term %.9g (fp64 %.9g, rel %.1e), gradient %.2e of max' % (
            case, kind, smooth, focal, got4[0], want4[0], abs(got4[0] - want4[0]) / max(abs(want4[0]), 1e-30), err))
        for name, a, b in zip(('box', 'wh', 'conf', 'class'), got4, want4):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (name, a, b)
        assert err < 2e-4
        n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
        _, y = IC.inputs(case)
        lanes = wantg.reshape(n, gh, gw, 3, 5 + C)[..., 0:4]
        assert (lanes[y[..., 4] == 0] == 0).all()        # exactly zero where there is no object, f[2] = 90 included
        assert want4[1] == 0.0


def test_box_loss_attribute_and_script_options():
    import yolov3_tensorflow_amd as y3
    model = y3.yolov3(3, COCO_ANCHORS)
    assert model.box_loss == 'mse'
    for name in ('giou', 'diou', 'ciou', 'mse'):
        model.box_loss = name
        assert model.box_loss == name
    for bad in ('iou', 'GIoU', 1, None):
        with pytest.raises(ValueError):
            model.box_loss = bad
    assert model.box_loss == 'mse'
    sys.path.insert(0, ROOT)
    try:
        import train
        assert train.build_parser().parse_args([]).box_loss == 'mse'
        assert train.build_parser().parse_args(['--box_loss', 'ciou']).box_loss == 'ciou'
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(['--box_loss', 'iou'])
        text = ' '.join(train.build_parser().format_help().split())
        assert '--box_loss' in text and '`xy` field holds the IoU box term' in text and '`wh` field is 0.00' in text
        src = open(os.path.join(ROOT, 'tools', 'train_bench.py')).read()
        assert "'--box_loss'" in src and 'model.box_loss = a.box_loss' in src
    finally:
        sys.path.remove(ROOT)


def test_library_refuses_an_unknown_kind_and_keeps_the_abi_version():
    """host-only: the setter on a net without a context"""
    import ctypes
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    assert L.y3_abi_version() == 5
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, 20, ctypes.byref(h)))
    try:
        for dtype in (0, 1, 4):
            _lib.check(L.y3_net_set_dtype(h, dtype))
            for kind in (1, 2, 3, 0):
                assert L.y3_net_train_set_box_loss(h, kind) == _lib.Y3_OK
        for kind in (4, -1):
            assert L.y3_net_train_set_box_loss(h, kind) == _lib.Y3_EINVAL
        assert L.y3_net_train_set_box_loss(None, 1) == _lib.Y3_EINVAL
    finally:
        L.y3_net_destroy(h)
