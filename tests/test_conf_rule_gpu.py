"""y3_loss_layer_conf (the ignore threshold and the IoU objectness target of the loss, include/yolo355.h) through the C ABI
against the fp64 oracle of tests/assign_cases.py, on the cases that module builds: less than one wave, a ragged chunk (tight and
padded gradient stride), unequal pixel-per-cell ratios, several workgroups, and more ground-truth boxes than the kernel stages
in the LDS; saturated object records and overflowing records without an object included.

Gates (the project's existing ones, test_loss_gpu.py): each term within 1e-4 * |ref| + 1e-6, the gradient within 2e-4 of the
tensor's max magnitude; test_assign_cpu.py shows that the oracle itself meets them in fp32.  The conditioning that keeps the
ignore mask's thresholds 0.3 / 0.5 / 0.7 from being crossed between fp32 and fp64 is assign_cases.inputs'."""
import numpy as np
import pytest
import torch

import assign_cases as AC
import test_loss_gpu as TL

pytestmark = pytest.mark.gpu

PARAMS = []
for _case in AC.CASE_NAMES:
    for _t, _r in AC.RULES:
        for _kind in ('mse', 'ciou'):
            for _smooth, _focal in AC.MODES:
                for _tight in ((False, True) if _case == '5x7_c20' else (False,)):
                    PARAMS.append(pytest.param(_case, _t, _r, _kind, _smooth, _focal, _tight,
                                               id='%s-t%g-r%g-%s-smooth%d-focal%d-%s' % (_case, _t, _r, _kind, _smooth, _focal,
                                                                                         'tight' if _tight else 'padded')))


@pytest.mark.parametrize('case,thresh,ratio,kind,smooth,focal,tight', PARAMS)
def test_loss_terms_and_gradient_match_the_fp64_oracle(case, thresh, ratio, kind, smooth, focal, tight):
    lanes, stride = TL._strides(case, tight)
    want4, wantg = AC.reference(case, kind, smooth, focal, thresh, ratio)
    rc, loss4, grad = AC.run_conf(case, kind, smooth, focal, thresh, ratio, stride)
    assert rc == 0
    gnp = grad.numpy()
    # every one of the 3F lanes is written and finite (the saturated and overflowing records included), the pad lanes are not
    assert np.isfinite(loss4.numpy()).all() and np.isfinite(gnp[..., :lanes]).all()
    assert np.isnan(gnp[..., lanes:]).all()
    AC.check_gates(loss4.tolist(), gnp[..., :lanes], want4, wantg, '%s %s t=%g r=%g smooth=%d focal=%d' % (
        case, kind, thresh, ratio, smooth, focal))
    # the rule changes the conf term and nothing else: the other three slots are y3_loss_layer_box's bits
    rc, base4, base_grad = AC.run_conf(case, kind, smooth, focal, 0.5, 0.0, stride, entry='box')
    assert rc == 0
    assert torch.equal(loss4[[0, 1, 3]], base4[[0, 1, 3]])
    if ratio > 0 or case == 'many_boxes':       # (a small case may hold no record between 0.5 and the threshold)
        assert not torch.equal(loss4[2], base4[2])
    F = lanes // 3
    conf_lane = np.arange(lanes) % F == 4
    assert np.array_equal(gnp[..., :lanes][..., ~conf_lane], base_grad.numpy()[..., :lanes][..., ~conf_lane])


@pytest.mark.parametrize('kind', ['mse', 'giou', 'diou', 'ciou'])
def test_the_defaults_are_y3_loss_layer_box_bit_for_bit(kind):
    for case in ('5x7_c20', 'many_boxes'):
        lanes, stride = TL._strides(case, False)
        for smooth, focal in AC.MODES:
            rc0, want4, wantg = AC.run_conf(case, kind, smooth, focal, 0.5, 0.0, stride, entry='box')
            rc1, got4, gotg = AC.run_conf(case, kind, smooth, focal, 0.5, 0.0, stride)
            assert rc0 == 0 and rc1 == 0
            assert torch.equal(got4.view(torch.int32), want4.view(torch.int32))
            assert torch.equal(gotg[..., :lanes].view(torch.int32), wantg[..., :lanes].view(torch.int32))


@pytest.mark.parametrize('case', ['5x7_c20', '20x28_c3'])
def test_accumulate_adds_to_what_loss4_held(case):
    lanes, stride = TL._strides(case, False)
    _, fresh, grad0 = AC.run_conf(case, 'ciou', True, False, 0.7, 1.0, stride)
    held = torch.tensor([1.5, -2.25, 1000.0, 3e-3], dtype=torch.float32)
    rc, got, grad1 = AC.run_conf(case, 'ciou', True, False, 0.7, 1.0, stride, accumulate=1, loss4=held.clone())
    assert rc == 0
    assert torch.equal(got, held + fresh)              # one fp32 addition per term: bit for bit
    assert torch.equal(grad0[..., :lanes], grad1[..., :lanes])


@pytest.mark.parametrize('thresh,ratio', [(-0.01, 0.0), (1.01, 0.0), (float('nan'), 0.0), (0.5, -0.01), (0.5, 1.01),
                                          (0.5, float('nan')), (float('inf'), 1.0)])
def test_out_of_range_values_are_refused_before_any_launch(thresh, ratio):
    from yolov3_tensorflow_amd import _lib
    case = '1x2_c1'
    lanes, stride = TL._strides(case, False)
    held = torch.tensor([1., 2., 3., 4.])
    rc, loss4, grad = AC.run_conf(case, 'mse', False, False, thresh, ratio, stride, loss4=held.clone())
    assert rc == _lib.Y3_EINVAL
    assert torch.equal(loss4, held) and bool(torch.isnan(grad).all())
    # the ends of the range are values like any other
    for t, r in ((0.0, 0.0), (1.0, 1.0)):
        rc, loss4, grad = AC.run_conf(case, 'mse', False, False, t, r, stride)
        assert rc == 0 and bool(torch.isfinite(loss4).all())


def test_guard_bands_of_the_tight_5x7_c20_call():
    """the entry assign_cases.py adds to test_guard_bands_gpu.py's table, through that module's own test"""
    import test_guard_bands_gpu as TG
    mine = [e for e in TG.TABLE if 'y3_loss_layer_conf' in e.covers]
    assert len(mine) == 1 and 'y3_net_train_set_conf_rule' in TG.EXCLUDED
    TG.test_guard_bands(mine[0])
