"""y3_loss_layer_box (include/yolo355.h: the loss of one scale with a GIoU / DIoU / CIoU box term, and its analytic gradient)
through the C ABI against the fp64 oracle of tests/iou_loss_cases.py, on the cases that module builds: less than one wave, a
full chunk plus a ragged one with a tight and a padded gradient stride, ratio_h != ratio_w, several workgroups, more
ground-truth boxes than the LDS stages; disjoint and enclosing boxes, saturated object records, and records without an object
whose exp(f) overflows and underflows.

Gates: the project's loss gates (tests/test_loss_gpu.py), each loss slot within 1e-4 |ref| + 1e-6 and the gradient within 2e-4
of the tensor's max magnitude.  What fp32 arithmetic alone costs on these inputs (the oracle evaluated by torch in fp32,
test_iou_loss_cpu.py): box term 1e-7 relative, gradient at most 1.9e-6 of max (many_boxes).

Measured on an MI355X (worst over the cases and both modes; the test prints every figure), the device's expf / atanf included:
  giou  box term 1.1e-7 relative (1x2_c1),   gradient 1.10e-6 of max (many_boxes)
  diou  box term 6.3e-8 relative (1x2_c1),   gradient 1.85e-6 of max (many_boxes)
  ciou  box term 6.5e-8 relative (20x28_c3), gradient 1.82e-6 of max (many_boxes)
which is where torch's fp32 evaluation sits: both gates hold with a factor of 100 to spare and none is widened."""
import ctypes

import numpy as np
import pytest
import torch

import iou_loss_cases as IC
import test_loss_gpu as TL

pytestmark = pytest.mark.gpu

PARAMS = []
for _case in IC.CASE_NAMES:
    for _tight in ((False, True) if _case == '5x7_c20' else (False,)):
        for _kind in sorted(IC.KINDS):
            for _mode in IC.MODES:
                PARAMS.append(pytest.param(_case, _kind, _mode[0], _mode[1], _tight, id='%s-%s-smooth%d-focal%d-%s' % (
                    _case, _kind, _mode[0], _mode[1], 'tight' if _tight else 'padded')))
CASE_MODES = [pytest.param(c, m[0], m[1], id='%s-smooth%d-focal%d' % (c, m[0], m[1])) for c in IC.CASE_NAMES for m in IC.MODES]

_MSE = {}


def run(case, kind, smooth, focal, grad_stride, accumulate=0, loss4=None, scratch=None, entry='y3_loss_layer_box'):
    """One call: grad pre-filled with NaN, the scratch (unless handed in) with 0xFF.  kind: a name, or the integer itself."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    fm, y = IC.inputs(case)
    fmg, yg = torch.from_numpy(fm).to(dev), torch.from_numpy(y).to(dev)
    grad = torch.full((n, gh, gw, grad_stride), float('nan'), device=dev)
    loss4 = torch.full((4,), float('nan'), device=dev) if loss4 is None else loss4
    if scratch is None:
        scratch = torch.full((L.y3_loss_scratch_bytes(n, gh, gw),), 0xFF, dtype=torch.uint8, device=dev)
    anc = np.ascontiguousarray(TL._anchors(scale), np.float32)
    head = (fw.context(), fw.ptr(fmg), fw.ptr(yg), n, gh, gw, C, H, W, anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            int(smooth), int(focal))
    tail = (accumulate, fw.ptr(loss4), fw.ptr(grad), grad_stride, fw.ptr(scratch), ctypes.c_size_t(scratch.numel()))
    if entry == 'y3_loss_layer':
        _lib.check(L.y3_loss_layer(*(head + tail)))
    else:
        _lib.check(L.y3_loss_layer_box(*(head + (IC.KINDS.get(kind, kind),) + tail)))
    torch.cuda.synchronize()
    return loss4.cpu(), grad.cpu(), scratch


def mse(case, smooth, focal, stride):
    """the box_loss = 0 call on the same inputs, once per (case, mode, stride)"""
    key = (case, smooth, focal, stride)
    if key not in _MSE:
        _MSE[key] = run(case, 0, smooth, focal, stride)[:2]
    return _MSE[key]


def records(case, grad, lanes):
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    return grad[..., :lanes].reshape(n, gh, gw, 3, 5 + C)


@pytest.mark.parametrize('case,kind,smooth,focal,tight', PARAMS)
def test_box_term_and_gradient_match_the_fp64_oracle(case, kind, smooth, focal, tight):
    lanes, stride = TL._strides(case, tight)
    want4, wantg = IC.reference(case, kind, smooth, focal)
    loss4, grad, scratch = run(case, kind, smooth, focal, stride)
    gnp = grad.numpy()
    got4 = loss4.tolist()
    print('%s %s smooth=%d focal=%d stride=%d: loss %s (ref %s), box term rel err %.2e, grad err %.2e of max' % (
        case, kind, smooth, focal, stride, got4, want4, abs(got4[0] - want4[0]) / abs(want4[0]), TL.rel_err(gnp[..., :lanes], wantg)))
    # every one of the 3F lanes is written and finite, the pad lanes behind them are not touched
    assert np.isfinite(gnp[..., :lanes]).all() and np.isfinite(got4).all()
    assert np.isnan(gnp[..., lanes:]).all()
    for name, a, b in zip(('box', 'wh', 'conf', 'class'), got4, want4):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (name, a, b)
    assert got4[1] == 0.0
    assert TL.rel_err(gnp[..., :lanes], wantg) < 2e-4
    # exactly zero in the four box lanes of every record without an object (f[2] = 90 and f[3] = -90 among them)
    _, y = IC.inputs(case)
    rec = records(case, gnp, lanes)
    assert (rec[..., 0:4][y[..., 4] == 0] == 0).all()
    # conf and class: the same bits as under box_loss = 0
    loss4m, gradm = mse(case, smooth, focal, stride)
    assert torch.equal(loss4[2:], loss4m[2:])
    assert np.array_equal(rec[..., 4:], records(case, gradm.numpy(), lanes)[..., 4:])
    assert not np.array_equal(rec[..., 0:4], records(case, gradm.numpy(), lanes)[..., 0:4])
    # again, on the scratch as the first call left it: the same bits
    loss4b, gradb, _ = run(case, kind, smooth, focal, stride, scratch=scratch)
    assert torch.equal(loss4, loss4b)
    assert torch.equal(grad[..., :lanes], gradb[..., :lanes])


@pytest.mark.parametrize('case,smooth,focal', CASE_MODES)
def test_kind_0_is_y3_loss_layer_bit_for_bit(case, smooth, focal):
    lanes, stride = TL._strides(case, False)
    loss4m, gradm = mse(case, smooth, focal, stride)
    loss4, grad, _ = run(case, None, smooth, focal, stride, entry='y3_loss_layer')
    assert bool(torch.isfinite(loss4).all()) and float(loss4[1]) > 0
    assert torch.equal(loss4, loss4m)
    assert torch.equal(grad[..., :lanes], gradm[..., :lanes])
    assert bool(torch.isnan(grad[..., lanes:]).all())


@pytest.mark.parametrize('kind', sorted(IC.KINDS))
@pytest.mark.parametrize('case', ['5x7_c20', '20x28_c3'])
def test_accumulate_adds_to_what_loss4_held(case, kind):
    from yolov3_tensorflow_amd import framework as fw
    lanes, stride = TL._strides(case, False)
    fresh, grad0, _ = run(case, kind, True, False, stride)
    held = torch.tensor([1.5, -2.25, 1000.0, 3e-3], dtype=torch.float32)
    got, grad1, _ = run(case, kind, True, False, stride, accumulate=1, loss4=held.clone().to(fw.default_device()))
    assert torch.equal(got, held + fresh)              # one fp32 addition per slot: bit for bit (the wh slot adds 0.0)
    assert torch.equal(grad0[..., :lanes], grad1[..., :lanes])


@pytest.mark.parametrize('kind', [4, -1])
def test_an_unknown_kind_is_refused_before_any_launch(kind):
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    case = '5x7_c20'
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    lanes, stride = TL._strides(case, False)
    fm, y = IC.inputs(case)
    fmg, yg = torch.from_numpy(fm).to(dev), torch.from_numpy(y).to(dev)
    loss4 = torch.full((4,), float('nan'), device=dev)
    grad = torch.full((n, gh, gw, stride), float('nan'), device=dev)
    scratch = torch.full((L.y3_loss_scratch_bytes(n, gh, gw),), 0xFF, dtype=torch.uint8, device=dev)
    anc = np.ascontiguousarray(TL._anchors(scale), np.float32)
    rc = L.y3_loss_layer_box(fw.context(), fw.ptr(fmg), fw.ptr(yg), n, gh, gw, C, H, W,
                             anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 0, 0, kind, 0, fw.ptr(loss4), fw.ptr(grad), stride,
                             fw.ptr(scratch), ctypes.c_size_t(scratch.numel()))
    torch.cuda.synchronize()
    assert rc == _lib.Y3_EINVAL
    with pytest.raises(ValueError):
        _lib.check(rc)
    # nothing was launched: grad, loss4 and the scratch hold what they held
    assert bool(torch.isnan(grad).all()) and bool(torch.isnan(loss4).all()) and bool((scratch == 0xFF).all())


def test_guard_bands_of_the_tight_5x7_c20_call():
    """the entry iou_loss_cases.py adds to test_guard_bands_gpu.py's table, through that module's own test: two passes on
    poisoned guards, outputs and scratch; no guard byte changed, the passes bit-identical, the oracle's gates"""
    import test_guard_bands_gpu as TG
    mine = [e for e in TG.TABLE if 'y3_loss_layer_box' in e.covers]
    assert len(mine) == 1 and 'y3_net_train_set_box_loss' in TG.EXCLUDED
    TG.test_guard_bands(mine[0])
