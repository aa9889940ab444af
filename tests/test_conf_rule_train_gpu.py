"""The conf rule in the one-call train step: y3_net_train_set_conf_rule, then y3_net_train_step, on the net of
tests/test_iou_loss_train_gpu.py (2 x 96 x 96, 20 classes; fp32 and the bf16 mixed-precision step, whose loss is fp32 too), and
the same through yolov3.ignore_thresh / yolov3.obj_iou_ratio with training.Trainer and compute_loss.  As there, nothing is
compared with an oracle - tests/test_conf_rule_gpu.py holds the per-scale entry to it: this file holds the step to the per-scale
entry, bit for bit, and the detection convs' bias gradients to the fp64 column sums of that entry's gradient, at the project's
gradient gate of 2e-4 of the max magnitude."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
import assign_cases as AC
import test_iou_loss_train_gpu as TI
import test_loss_gpu as TL

pytestmark = pytest.mark.gpu

N, HW, C, DET, DET_PAD = TI.N, TI.HW, TI.C, TI.DET, TI.DET_PAD
RULE = (0.7, 1.0)


def per_scale(fms, yts, kind, thresh, ratio):
    """compute_loss as three accumulating y3_loss_layer_conf calls: ([total, box, wh, conf, class] as the library sums them,
    the three gradients [n, g, g, DET_PAD])"""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    loss4 = torch.zeros(4, device=dev)
    grads = []
    for i, (fm, y) in enumerate(zip(fms, yts)):
        g = fm.shape[1]
        grad = torch.zeros((N, g, g, DET_PAD), device=dev)
        sc = torch.full((L.y3_loss_scratch_bytes(N, g, g),), 0xFF, dtype=torch.uint8, device=dev)
        anc = np.ascontiguousarray(COCO_ANCHORS[6 - 3 * i:9 - 3 * i], np.float32)
        _lib.check(L.y3_loss_layer_conf(fw.context(), fw.ptr(fm), fw.ptr(y), N, g, g, C, HW, HW,
                                        anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), TI.SMOOTH, TI.FOCAL, kind,
                                        ctypes.c_float(thresh), ctypes.c_float(ratio), int(i > 0), fw.ptr(loss4), fw.ptr(grad),
                                        DET_PAD, fw.ptr(sc), ctypes.c_size_t(sc.numel())))
        grads.append(grad)
    torch.cuda.synchronize()
    l = loss4.cpu().numpy()
    total = np.float32(np.float32(np.float32(l[0] + l[1]) + l[2]) + l[3])          # xy + wh + conf + class, in this order
    return torch.from_numpy(np.array([total, l[0], l[1], l[2], l[3]], np.float32)), [g.cpu() for g in grads]


def _set(s, thresh, ratio):
    return s.L.y3_net_train_set_conf_rule(s.h, ctypes.c_float(thresh), ctypes.c_float(ratio))


@pytest.mark.parametrize('dtype,kind', [('f32', 'mse'), ('f32', 'ciou'), ('bf16', 'ciou')])
def test_step_with_a_conf_rule_is_the_per_scale_entry_on_its_feature_maps(dtype, kind, isolated_graph):
    s = TI._Step(dtype)
    k = AC.KINDS[kind]
    try:
        ws_bytes = s.L.y3_net_train_workspace_bytes(s.h, s.table, N, HW, HW)
        # a net that never called the setter, and one set to (0.5, 0): the same loss5 and flat_grad bits
        base5, base_flat = s.step(k)
        assert _set(s, 0.5, 0.0) == 0
        again5, again_flat = s.step(k)
        assert torch.equal(base5.view(torch.int32), again5.view(torch.int32))
        assert torch.equal(base_flat.view(torch.int32), again_flat.view(torch.int32))
        assert _set(s, *RULE) == 0
        assert s.L.y3_net_train_workspace_bytes(s.h, s.table, N, HW, HW) == ws_bytes
        loss5, flat = s.step(k)
        assert bool(torch.isfinite(loss5).all()) and bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        fms = s.feature_maps()
        want5, grads = per_scale(fms, s.yts, k, *RULE)
        print('%s %s: loss5 %s (defaults %s)' % (dtype, kind, loss5.tolist(), base5.tolist()))
        assert torch.equal(loss5, want5)
        assert torch.equal(base5, per_scale(fms, s.yts, k, 0.5, 0.0)[0])
        assert torch.equal(base5, TI.per_scale(fms, s.yts, k)[0])
        # the box and class terms do not know the rule; the conf term does
        assert torch.equal(loss5[[1, 2, 4]], base5[[1, 2, 4]]) and float(loss5[3]) != float(base5[3])
        # the detection convs' bias gradients: column sums of d loss / d feature map
        biases = [lv[2] for lv in s.layer_vars if lv[2] is not None]
        assert len(biases) == 3
        for b, g in zip(biases, grads):
            off = s.offsets[b.op_name]
            got = flat[off:off + DET].numpy()
            want = g[..., :DET].double().sum(dim=(0, 1, 2)).numpy()
            err = TL.rel_err(got.astype(np.float64), want)
            print('  %s: bias gradient %.2e of max from the column sums' % (b.op_name, err))
            assert np.abs(want).max() > 0 and err < 2e-4
        # a second step: the same bits; the gradient is not the default step's; (0.5, 0) again is the default step again
        loss5b, flatb = s.step(k)
        assert torch.equal(loss5, loss5b) and torch.equal(flat, flatb)
        assert not torch.equal(flat, base_flat)
        # bad values are refused and the net keeps BOTH values it had
        for bad in ((-0.1, 0.0), (1.1, 0.0), (float('nan'), 0.0), (0.5, -0.1), (0.5, 1.5), (0.5, float('nan')), (0.3, 2.0)):
            assert _set(s, *bad) == s._lib.Y3_EINVAL
        loss5c, _ = s.step(k)
        assert torch.equal(loss5, loss5c)
        assert _set(s, 0.5, 0.0) == 0
        back5, back_flat = s.step(k)
        assert torch.equal(base5, back5) and torch.equal(base_flat, back_flat)
    finally:
        s.destroy()


def test_model_conf_rule_through_trainer_and_compute_loss(isolated_graph):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    s = TI._Step('f32')
    try:
        raw = {}
        for rule in ((0.5, 0.0), RULE, (0.3, 0.5)):
            assert _set(s, *rule) == 0
            raw[rule] = s.step(AC.KINDS['ciou'])[0]
    finally:
        s.destroy()
    model = s.model
    model.box_loss = 'ciou'
    # a learning rate of 0 (sgd: w -= 0 * g) keeps the variables, so one Trainer can take the same step under each rule
    trainer = training.Trainer(model, config_optimizer('sgd', 0.0), wgrad_stream=False)
    got = {}
    with y3.variable_scope('yolov3'):
        for rule in ((0.5, 0.0), RULE, (0.5, 0.0), (0.3, 0.5)):
            model.ignore_thresh, model.obj_iou_ratio = rule
            loss = trainer.step(s.x, s.yts)
            torch.cuda.synchronize()
            cur = (torch.stack(loss).cpu(), trainer.flat.clone().cpu())
            assert bool(torch.isfinite(cur[1]).all())
            assert torch.equal(cur[0], raw[rule]), rule
            if rule in got:                    # back to the defaults: the first step bit for bit
                assert torch.equal(cur[1], got[rule][1])
            got[rule] = cur
        assert not torch.equal(got[RULE][1], got[(0.5, 0.0)][1]) and not torch.equal(got[(0.3, 0.5)][1], got[RULE][1])
        # compute_loss on the maps of a training forward: the train net, which follows the attributes at every call
        model.ignore_thresh, model.obj_iou_ratio = RULE
        fms = model.forward(s.x, is_training=True)
        assert torch.equal(torch.stack(model.compute_loss(fms, s.yts)).cpu(), raw[RULE])
        model.ignore_thresh, model.obj_iou_ratio = 0.3, 0.5
        assert torch.equal(torch.stack(model.compute_loss(fms, s.yts)).cpu(), raw[(0.3, 0.5)])
        # the validation path: the maps of forward(is_training=False) go through the per-scale entry
        fms = [f.clone() for f in model.forward(s.x, is_training=False)]
        loss = torch.stack(model.compute_loss(fms, s.yts)).cpu()
        want5, _ = per_scale(fms, s.yts, AC.KINDS['ciou'], 0.3, 0.5)
        assert torch.equal(loss[1:], want5[1:])
        assert abs(float(loss[0]) - float(want5[0])) <= 1e-6 * abs(float(want5[0]))      # (summed by torch there)
        x4 = model.loss_layer(fms[0], s.yts[0], COCO_ANCHORS[6:9])
        model.ignore_thresh, model.obj_iou_ratio = 0.5, 0.0
        d4 = model.loss_layer(fms[0], s.yts[0], COCO_ANCHORS[6:9])
        assert float(x4[0]) == float(d4[0]) and float(x4[3]) == float(d4[3]) and float(x4[2]) != float(d4[2])
