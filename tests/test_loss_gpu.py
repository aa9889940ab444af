"""y3_loss_layer (the loss of one scale and its gradient, ref: model.py:192-345) through the C ABI against the fp64 autograd
oracle (oracle/train_ref.py: TrainGraph.loss_layer, gradient = backward of the sum of the four terms), away from the
80-class, square, mix-up-weight-1 regime of test_train_gpu.py: non-square grids, mix-up weights in (0.2, 1), 1 / 2 / 3 / 20 /
80 classes, saturated logits that enter both tf.clip_by_value branches, all four (label_smooth, focal) combinations, a tight
and a padded gradient row stride, accumulate, uninitialised scratch, and an image with more ground-truth boxes than the
kernel stages in the LDS.

What shows which transposition: every COCO anchor has w != h and the non-square grids have gh != gw, so an exchange of
anc_w / anc_h, img_w / img_h or gx / gy shows in every non-square case.  The two pixel-per-cell ratios do not: wherever the
image is grid * stride, ratio_h == ratio_w bit for bit and an exchange of the two computes the same thing.  y3_loss_layer
takes the image size independently of the grid, so 5x7_r30x32 gives it a 150 x 224 image on the 5 x 7 grid (ratio_h 30,
ratio_w 32); that case is the one that fails when ratio_w and ratio_h are exchanged in loss_kernel's px / py lines.

Conventions: the oracle's img_size is [H, W]; process_box and synthetic_targets take [W, H].

Gates (the project's existing ones, test_train_gpu.py): each loss term within 1e-4 * |ref| + 1e-6, the gradient within 2e-4
of the tensor's max magnitude.

Conditioning: the ignore mask is a threshold (best IoU < 0.5); a record that crosses it between fp32 and fp64 moves its conf
term by O(1).  The fp32 IoU is good to about 1e-6, so the inputs are built such that no record's fp64 best IoU lies within
1e-4 of 0.5 (100x headroom): a record that does has its f[2], f[3] redrawn, and the builder then asserts the condition.  No
record is left out of any comparison."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS

pytestmark = pytest.mark.gpu

IOU_MARGIN = 1e-4

# name: (n, gh, gw, img H, img W, classes, scale (0: stride 32, anchors 6:9; 1: stride 16; 2: stride 8), target seed).
# The seeds are ones whose synthetic_targets put objects on the tested scale in the images that keep theirs (8, 2, 3 and 3
# object records in the four cases that take them from there; 5x7_c20 needs four for the saturated logits; 5x7_r30x32 has
# the targets of 5x7_c20).
CASES = {
    '1x2_c1': (2, 1, 2, 32, 64, 1, 0, 11),         # 6 records: less than one wave.  F = 6
    '5x7_c20': (3, 5, 7, 160, 224, 20, 0, 7),      # 105 records: a full 64-record chunk and a ragged one.  F = 25
    '5x7_r30x32': (3, 5, 7, 150, 224, 20, 0, 7),   # the same targets, squeezed to 150 rows: ratio_h = 30, ratio_w = 32
    '10x14_c20': (2, 10, 14, 160, 224, 20, 1, 1),  # the middle scale of the same input
    '20x28_c3': (2, 20, 28, 160, 224, 3, 2, 50),   # 1680 records: several workgroups.  F = 8
    '13x13_c80': (1, 13, 13, 416, 416, 80, 0, 5),  # the regime of test_train_gpu.py, now with mix-up weights
    'many_boxes': (2, 32, 32, 256, 256, 2, 2, 16),  # 2500 ground-truth boxes in one image: more than the LDS stages (2048)
}
ALL_MODES = [(False, False), (False, True), (True, False), (True, True)]
PARAMS = []
for _name in CASES:
    for _mode in (ALL_MODES if _name in ('5x7_c20', '13x13_c80') else [(False, False), (True, True)]):
        for _tight in ((False, True) if _name == '5x7_c20' else (False,)):
            PARAMS.append(pytest.param(_name, _mode[0], _mode[1], _tight,
                                       id='%s-smooth%d-focal%d-%s' % (_name, _mode[0], _mode[1], 'tight' if _tight else 'padded')))

_INPUTS, _REFS = {}, {}


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))


def _anchors(scale):
    return COCO_ANCHORS[6 - 3 * scale:9 - 3 * scale]


def _graph(case):
    from oracle import train_ref
    n, gh, gw, H, W, C, scale, seed = CASES[case]
    g = train_ref.TrainGraph({}, C, torch.float64)
    g.img_size = [H, W]
    return g


def best_iou64(case, fm, y):
    """[n, gh, gw, 3] fp64 best IoU of every record with the ground-truth boxes of its image (-inf where it has none)"""
    from oracle import train_ref
    scale = CASES[case][6]
    g = _graph(case)
    _, pred, _, _ = g.reorg(torch.tensor(fm, dtype=torch.float64), _anchors(scale))
    yt = torch.tensor(y, dtype=torch.float64)
    out = np.full(y.shape[:4], -np.inf)
    for i in range(y.shape[0]):
        valid = yt[i, ..., 0:4][yt[i, ..., 4] > 0.5]
        if valid.shape[0]:
            out[i] = train_ref.TrainGraph.box_iou(pred[i], valid).max(dim=-1).values.numpy()
    return out


def _targets(case):
    from oracle import train_ref
    n, gh, gw, H, W, C, scale, seed = CASES[case]
    rng = np.random.RandomState(seed)
    if case == 'many_boxes':
        # y_true written directly: image 0 has 2500 object records (of 3072), each with a centre inside its own cell, a size
        # around this scale's anchors, a one-hot class and a mix-up weight; image 1 has none
        y = np.zeros((n, gh, gw, 3, 6 + C), np.float32)
        y[..., -1] = 1.
        rec = rng.choice(gh * gw * 3, 2500, replace=False)
        cy, cx, k = np.unravel_index(rec, (gh, gw, 3))
        y[0, cy, cx, k, 0] = (cx + rng.uniform(0, 1, 2500)) * (W / gw)
        y[0, cy, cx, k, 1] = (cy + rng.uniform(0, 1, 2500)) * (H / gh)
        y[0, cy, cx, k, 2] = rng.uniform(6, 60, 2500)
        y[0, cy, cx, k, 3] = rng.uniform(6, 60, 2500)
        y[0, cy, cx, k, 4] = 1.
        y[0, cy, cx, k, 5 + rng.randint(0, C, 2500)] = 1.
        y[0, cy, cx, k, -1] = rng.uniform(0.2, 1.0, 2500)
        return y
    # (boxes small enough for the stride-8 anchors are rare among w, h ~ U(10, 300): more draws there)
    stride = 32 >> scale
    y = train_ref.synthetic_targets(seed, n, [gw * stride, gh * stride], C, COCO_ANCHORS, max_boxes=24 if scale == 2 else 8,
                                    mix_up=(0.2, 1.0))[scale]
    if H != gh * stride:                        # squeeze the boxes (cy, h) into the H rows: each centre stays in its cell
        y[..., 1] *= np.float32(H / (gh * stride))
        y[..., 3] *= np.float32(H / (gh * stride))
    if n > 1:                                   # one image of the batch has no object on this scale
        y[n - 1] = 0
        y[n - 1][..., -1] = 1
    if case == '1x2_c1':
        # a 64 x 32 image holds no box as large as the stride-32 anchors, so synthetic_targets (through process_box's best
        # anchor) leaves this scale empty: one record is written directly, as process_box would write it - a 50 x 28 box
        # inside the image, in the cell of its centre, on the scale's first anchor, with a mix-up weight
        assert y[..., 4].sum() == 0
        y[0, 0, 1, 0, :] = [41., 15., 50., 28., 1., 1., 0.6]
    return y


def inputs(case):
    """(logits [n, gh, gw, 3F] fp32, y_true [n, gh, gw, 3, 6+C] fp32) of a case, built once on the CPU"""
    if case in _INPUTS:
        return _INPUTS[case]
    n, gh, gw, H, W, C, scale, seed = CASES[case]
    F = 5 + C
    y = _targets(case)
    assert y[0, ..., 4].sum() > 0 and (n == 1 or y[n - 1, ..., 4].sum() == 0)
    rng = np.random.RandomState(1000 + seed)
    fm = (rng.standard_normal((n, gh, gw, 3, F)) * 1.5).astype(np.float32)
    if case == '5x7_c20':
        # saturated logits on four object records.  ln 1e9 = 20.7: +25 / -25 put pred_twth outside tf.clip_by_value's
        # [1e-9, 1e9] on either side (zero gradient there), in fp32 and fp64 alike; +-40 drive bce_ to its two asymptotes
        obj = np.argwhere(y[..., 4] > 0.5)
        assert len(obj) >= 4, len(obj)
        r0, r1, r2, r3 = [tuple(o) for o in obj[:4]]
        fm[r0][2] = 25.
        fm[r1][3] = -25.
        fm[r2][4] = 40.
        fm[r3][4] = -40.
        fm[r3][5 + (int(np.argmax(y[r3][5:5 + C])) + 1) % C] = 40.        # a class logit that is NOT the target
    best = best_iou64(case, fm.reshape(n, gh, gw, 3 * F), y)
    for _ in range(20):
        close = np.abs(best - 0.5) < IOU_MARGIN
        if not close.any():
            break
        fm[close, 2:4] = (rng.standard_normal((int(close.sum()), 2)) * 1.5).astype(np.float32)
        best = best_iou64(case, fm.reshape(n, gh, gw, 3 * F), y)
    assert not (np.abs(best - 0.5) < IOU_MARGIN).any()
    if case == 'many_boxes':                      # the mask must be decided by boxes on both sides of the threshold
        assert (best[0] >= 0.5).sum() > 100 and (best[0] < 0.5).sum() > 100
    _INPUTS[case] = (fm.reshape(n, gh, gw, 3 * F), y)
    return _INPUTS[case]


def reference(case, smooth, focal):
    """([xy, wh, conf, class] fp64, d(sum)/d(logits) fp64), computed once per (case, mode)"""
    key = (case, smooth, focal)
    if key not in _REFS:
        fm, y = inputs(case)
        t = torch.tensor(fm, dtype=torch.float64, requires_grad=True)
        parts = _graph(case).loss_layer(t, y, _anchors(CASES[case][6]), smooth, focal)
        sum(parts).backward()
        _REFS[key] = ([float(p.detach()) for p in parts], t.grad.numpy())
    return _REFS[key]


def run(case, smooth, focal, grad_stride, accumulate=0, loss4=None, scratch=None, scratch_bytes=None):
    """One y3_loss_layer call: grad pre-filled with NaN, the scratch (unless handed in) with 0xFF."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    n, gh, gw, H, W, C, scale, seed = CASES[case]
    fm, y = inputs(case)
    fmg, yg = torch.from_numpy(fm).to(dev), torch.from_numpy(y).to(dev)
    grad = torch.full((n, gh, gw, grad_stride), float('nan'), device=dev)
    loss4 = torch.full((4,), float('nan'), device=dev) if loss4 is None else loss4
    if scratch is None:
        scratch = torch.full((L.y3_loss_scratch_bytes(n, gh, gw),), 0xFF, dtype=torch.uint8, device=dev)
    anc = np.ascontiguousarray(_anchors(scale), np.float32)
    _lib.check(L.y3_loss_layer(fw.context(), fw.ptr(fmg), fw.ptr(yg), n, gh, gw, C, H, W,
                               anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(smooth), int(focal), accumulate,
                               fw.ptr(loss4), fw.ptr(grad), grad_stride, fw.ptr(scratch),
                               ctypes.c_size_t(scratch.numel() if scratch_bytes is None else scratch_bytes)))
    torch.cuda.synchronize()
    return loss4.cpu(), grad.cpu(), scratch


def _strides(case, tight):
    lanes = 3 * (5 + CASES[case][5])
    return lanes, lanes if tight else ((lanes + 31) // 32) * 32


@pytest.mark.parametrize('case,smooth,focal,tight', PARAMS)
def test_loss_terms_and_gradient_match_the_fp64_oracle(case, smooth, focal, tight):
    """many_boxes on the library before the LDS limit was lifted (best IoU over an arbitrary 2048 of the 2500 boxes): the conf
    term and the gradient miss these gates, and the two calls differ."""
    lanes, stride = _strides(case, tight)
    want4, wantg = reference(case, smooth, focal)
    loss4, grad, scratch = run(case, smooth, focal, stride)
    gnp = grad.numpy()
    print('%s smooth=%d focal=%d stride=%d: loss %s (ref %s), grad rel err %.2e' % (
        case, smooth, focal, stride, loss4.tolist(), want4, rel_err(gnp[..., :lanes], wantg)))
    # every one of the 3F lanes is written, the pad lanes behind them are not
    assert np.isfinite(gnp[..., :lanes]).all()
    assert np.isnan(gnp[..., lanes:]).all()
    for name, a, b in zip(('xy', 'wh', 'conf', 'class'), loss4.tolist(), want4):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (name, a, b)
    assert rel_err(gnp[..., :lanes], wantg) < 2e-4
    # again, on the scratch as the first call left it: the same bits
    loss4b, gradb, _ = run(case, smooth, focal, stride, scratch=scratch)
    assert torch.equal(loss4, loss4b)
    assert torch.equal(grad[..., :lanes], gradb[..., :lanes])


@pytest.mark.parametrize('case', ['5x7_c20', '20x28_c3'])
def test_accumulate_adds_to_what_loss4_held(case):
    from yolov3_tensorflow_amd import framework as fw
    lanes, stride = _strides(case, False)
    fresh, grad0, _ = run(case, True, False, stride)
    held = torch.tensor([1.5, -2.25, 1000.0, 3e-3], dtype=torch.float32)
    got, grad1, _ = run(case, True, False, stride, accumulate=1, loss4=held.clone().to(fw.default_device()))
    assert torch.equal(got, held + fresh)              # one fp32 addition per term: bit for bit
    assert torch.equal(grad0[..., :lanes], grad1[..., :lanes])


def test_short_gradient_rows_and_a_short_scratch_are_refused():
    from yolov3_tensorflow_amd import _lib
    case = '5x7_c20'
    n, gh, gw = CASES[case][:3]
    lanes, stride = _strides(case, True)
    with pytest.raises(ValueError):
        run(case, False, False, lanes - 1)
    with pytest.raises(ValueError):
        run(case, False, False, stride, scratch_bytes=_lib.lib().y3_loss_scratch_bytes(n, gh, gw) - 1)
