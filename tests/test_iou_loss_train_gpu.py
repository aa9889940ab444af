"""The IoU box losses in the one-call train step: y3_net_train_set_box_loss, then y3_net_train_step, on one net (2 x 96 x 96,
20 classes; fp32 and the bf16 mixed-precision step, whose loss is fp32 too), and the same through yolov3.box_loss with
training.Trainer and compute_loss.  Nothing here is compared with an oracle - tests/test_iou_loss_gpu.py holds the per-scale
entry to it, tests/test_train_gpu.py the step's backward: this file holds the step to the per-scale entry, bit for bit, and
the detection convs' bias gradients (the first thing backward makes of d loss / d feature map) to the fp64 column sums of that
entry's gradient, at the project's gradient gate of 2e-4 of the max magnitude."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS, blob_images
import iou_loss_cases as IC
import test_loss_gpu as TL
import test_train_gpu as TT

pytestmark = pytest.mark.gpu

N, HW, C = 2, 96, 20
DET = 3 * (5 + C)
DET_PAD = ((DET + 31) // 32) * 32
SMOOTH, FOCAL = 1, 1


@functools.lru_cache(maxsize=None)
def _data():
    from oracle import yolo_ref, train_ref
    params = yolo_ref.synthetic_params(C, seed=6)
    x = blob_images(5, N, HW)
    yts = train_ref.synthetic_targets(21, N, [HW, HW], C, COCO_ANCHORS, max_boxes=6, mix_up=(0.2, 1.0))
    assert sum(float(y[..., 4].sum()) for y in yts) >= 4
    return params, x, yts


class _Step(object):
    """A y3_net of its own on the variables of a fresh model, every variable trainable."""

    def __init__(self, dtype):
        import yolov3_tensorflow_amd as y3
        from yolov3_tensorflow_amd import framework as fw, _lib, training
        params, x, yts = _data()
        self.model = TT._fresh_model(params, class_num=C, batch_norm_decay=0.99, use_label_smooth=bool(SMOOTH),
                                     use_focal_loss=bool(FOCAL))
        self.model.compute_dtype = dtype
        self.L, self._lib, self.fw = _lib.lib(), _lib, fw
        self.dev = fw.default_device()
        self.x = torch.from_numpy(x).to(self.dev)
        self.yts = [torch.from_numpy(y).to(self.dev) for y in yts]
        with y3.variable_scope('yolov3'):
            _, _, self.layer_vars = training._prepare(self.model, self.x)
        self.order, self.offsets, _, self.total = training.gradient_layout(self.layer_vars)
        self.table, self.keep = training._var_table(self.layer_vars)
        # (the layout aligns each tensor: the elements between two tensors belong to no gradient and are never written)
        self.covered = torch.zeros(self.total, dtype=torch.bool)
        for v in self.order:
            self.covered[self.offsets[v.op_name]:self.offsets[v.op_name] + v.tensor.numel()] = True
        self.h = ctypes.c_void_p()
        _lib.check(self.L.y3_net_create(fw.context(), C, ctypes.byref(self.h)))
        _lib.check(self.L.y3_net_set_dtype(self.h, training._TRAIN_DTYPES[dtype]))
        wb = self.L.y3_net_train_workspace_bytes(self.h, self.table, N, HW, HW)
        assert wb > 0
        self.ws = torch.full((wb,), 0xFF, dtype=torch.uint8, device=self.dev)
        self.anc = np.ascontiguousarray(COCO_ANCHORS, np.float32)
        self.opts = _lib.TrainOpts(0.99, SMOOTH, FOCAL, self.anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def destroy(self):
        self.L.y3_net_destroy(self.h)

    def step(self, kind):
        """(loss5, flat_grad) of y3_net_train_set_box_loss(kind) + y3_net_train_step, both outputs pre-filled with NaN (what
        the layout leaves between two tensors must still hold it, and is returned as 0)"""
        fw, L = self.fw, self.L
        self._lib.check(L.y3_net_train_set_box_loss(self.h, kind))
        flat = torch.full((self.total,), float('nan'), device=self.dev)
        loss5 = torch.full((5,), float('nan'), device=self.dev)
        y = self.yts
        self._lib.check(L.y3_net_train_step(self.h, self.table, fw.ptr(self.x), N, HW, HW, fw.ptr(y[0]), fw.ptr(y[1]), fw.ptr(y[2]),
                                            ctypes.byref(self.opts), fw.ptr(flat), fw.ptr(self.ws), ctypes.c_size_t(self.ws.numel()),
                                            fw.ptr(loss5), self._lib.GradReadyFn(), None))
        torch.cuda.synchronize()
        flat = flat.cpu()
        assert bool(torch.isnan(flat[~self.covered]).all())
        return loss5.cpu(), torch.where(self.covered, flat, torch.zeros_like(flat))

    def feature_maps(self):
        """the step's feature maps: y3_net_train_forward on the same input leaves the same bits in the same workspace and
        returns where"""
        fw, L = self.fw, self.L
        fm = [ctypes.c_void_p() for _ in range(3)]
        self._lib.check(L.y3_net_train_forward(self.h, self.table, fw.ptr(self.x), N, HW, HW, ctypes.byref(self.opts), fw.ptr(self.ws),
                                               ctypes.c_size_t(self.ws.numel()), *[ctypes.byref(p) for p in fm]))
        torch.cuda.synchronize()
        out = []
        for p, s in zip(fm, (32, 16, 8)):
            o = p.value - self.ws.data_ptr()
            assert 0 <= o < self.ws.numel()
            g = HW // s
            out.append(self.ws[o:o + N * g * g * DET * 4].view(torch.float32).view(N, g, g, DET).clone())
        return out


def per_scale(fms, yts, kind, smooth=SMOOTH, focal=FOCAL):
    """compute_loss as three accumulating y3_loss_layer_box calls: ([total, box, wh, conf, class] as the library sums them,
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
        _lib.check(L.y3_loss_layer_box(fw.context(), fw.ptr(fm), fw.ptr(y), N, g, g, C, HW, HW,
                                       anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), smooth, focal, kind, int(i > 0),
                                       fw.ptr(loss4), fw.ptr(grad), DET_PAD, fw.ptr(sc), ctypes.c_size_t(sc.numel())))
        grads.append(grad)
    torch.cuda.synchronize()
    l = loss4.cpu().numpy()
    total = np.float32(np.float32(np.float32(l[0] + l[1]) + l[2]) + l[3])          # xy + wh + conf + class, in this order
    return torch.from_numpy(np.array([total, l[0], l[1], l[2], l[3]], np.float32)), [g.cpu() for g in grads]


@pytest.mark.parametrize('dtype,kind', [('f32', 'giou'), ('f32', 'ciou'), ('bf16', 'giou')])
def test_step_with_an_iou_kind_is_the_per_scale_entry_on_its_feature_maps(dtype, kind, isolated_graph):
    s = _Step(dtype)
    try:
        mse5, mse_flat = s.step(0)
        loss5, flat = s.step(IC.KINDS[kind])
        assert bool(torch.isfinite(loss5).all()) and bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        assert float(loss5[2]) == 0.0 and float(mse5[2]) > 0
        fms = s.feature_maps()
        want5, grads = per_scale(fms, s.yts, IC.KINDS[kind])
        print('%s %s: loss5 %s (mse %s)' % (dtype, kind, loss5.tolist(), mse5.tolist()))
        assert torch.equal(loss5, want5)
        assert torch.equal(mse5, per_scale(fms, s.yts, 0)[0])
        # conf and class do not know the kind
        assert torch.equal(loss5[3:], mse5[3:])
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
        # a second step: the same bits; the gradient is not the mse step's; kind 0 again is the mse step again
        loss5b, flatb = s.step(IC.KINDS[kind])
        assert torch.equal(loss5, loss5b) and torch.equal(flat, flatb)
        assert not torch.equal(flat, mse_flat)
        mse5b, mse_flatb = s.step(0)
        assert torch.equal(mse5, mse5b) and torch.equal(mse_flat, mse_flatb)
        # an unknown kind is refused and the net keeps the one it had
        assert s.L.y3_net_train_set_box_loss(s.h, 4) == s._lib.Y3_EINVAL
        mse5c, _ = s.step(0)
        assert torch.equal(mse5, mse5c)
    finally:
        s.destroy()


def test_model_box_loss_through_trainer_and_compute_loss(isolated_graph):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    s = _Step('f32')
    try:
        raw = {k: s.step(v)[0] for k, v in (('mse', 0),) + tuple(IC.KINDS.items())}
    finally:
        s.destroy()
    model = s.model
    # a learning rate of 0 (sgd: w -= 0 * g) keeps the variables, so one Trainer can take the same step under each kind
    trainer = training.Trainer(model, config_optimizer('sgd', 0.0), wgrad_stream=False)
    got = {}
    with y3.variable_scope('yolov3'):
        for name in ('mse', 'giou', 'mse', 'ciou'):
            model.box_loss = name
            loss = trainer.step(s.x, s.yts)
            torch.cuda.synchronize()
            cur = (torch.stack(loss).cpu(), trainer.flat.clone().cpu())
            assert bool(torch.isfinite(cur[1]).all())
            assert torch.equal(cur[0], raw[name]), name
            if name in got:                    # back to mse: the first mse step bit for bit
                assert torch.equal(cur[1], got[name][1])
            got[name] = cur
        assert not torch.equal(got['giou'][1], got['mse'][1]) and not torch.equal(got['ciou'][1], got['giou'][1])
        assert float(got['giou'][0][2]) == 0.0
        # compute_loss on the maps of a training forward: the train net, which follows the attribute at every call
        model.box_loss = 'giou'
        fms = model.forward(s.x, is_training=True)
        assert torch.equal(torch.stack(model.compute_loss(fms, s.yts)).cpu(), raw['giou'])
        model.box_loss = 'diou'
        assert torch.equal(torch.stack(model.compute_loss(fms, s.yts)).cpu(), raw['diou'])
        # the validation path: the maps of forward(is_training=False) go through the per-scale entry
        fms = [f.clone() for f in model.forward(s.x, is_training=False)]
        loss = torch.stack(model.compute_loss(fms, s.yts)).cpu()
        want5, _ = per_scale(fms, s.yts, IC.KINDS['diou'])
        assert torch.equal(loss[1:], want5[1:]) and float(loss[2]) == 0.0
        assert abs(float(loss[0]) - float(want5[0])) <= 1e-6 * abs(float(want5[0]))      # (summed by torch there)
        x4 = model.loss_layer(fms[0], s.yts[0], COCO_ANCHORS[6:9])
        assert float(x4[1]) == 0.0 and float(x4[0]) > 0
        model.box_loss = 'mse'
        assert float(model.compute_loss(fms, s.yts)[2]) > 0
