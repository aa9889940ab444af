"""Cases and oracles of the multi-anchor target assignment (include/yolo355.h at y3_process_box_multi) and of the conf rule
(y3_loss_layer_conf: ignore threshold and IoU objectness target), shared by test_assign_cpu.py, test_assign_gpu.py,
test_conf_rule_gpu.py, test_conf_rule_train_gpu.py and test_assign_feeder_gpu.py.

Assignment.  The oracle is the product's own utils.data_utils.process_box_host (plain numpy float32: the rule in executable
form); test_assign_cpu.py pins it to the reference's goldens at the default and to records worked by hand at darknet's 0.213.
The hand cases (COCO anchors): a 40 x 50 box has best anchor 3 and extras {1, 2, 4, 5}; 12 x 14 has best 0 and extras {1, 2};
300 x 280 has best 8 and extra {7}; 60 x 80 has best 5 and extras {3, 4, 6}.  gpu_case() keeps these SIZES (the shape IoUs
know nothing else of a box) and moves the centres into a 96 x 64 image, whose grids 3 x 2, 6 x 4 and 12 x 8 are not square.

Conf rule.  ConfGraph.loss_layer restates oracle.train_ref.TrainGraph.loss_layer in torch with (ignore_thresh, obj_iou_ratio)
and iou_loss_cases' box term: the target z = (1 - r) + r * q of an object record, q the plain IoU of the decoded prediction
with the record's own true box, detached, non-finite or negative values mapped to 0; z = 0 without an object, by selection.
The xy / wh terms decode with f[0:4] of the records without an object selected away first (as iou_loss_cases' IouGraph does
for its box term): those records contribute exactly 0 either way, and the oracle can then run in fp32 on logits whose exp
overflows.  At (0.5, 0) it is TrainGraph.loss_layer to the bit (test_assign_cpu.py).

The cases are iou_loss_cases' inputs (test_loss_gpu.CASES with the saturated object records f[2] = 25, f[3] = -25 of 5x7_c20,
two overflowing records without an object per case, the disjoint and the enclosing record of many_boxes), conditioned once
more, for all tested thresholds at once: the ignore mask is a threshold on the best IoU, and a record that crosses it between
fp32 and fp64 moves its conf term by O(1).  The fp32 IoU is good to about 1e-6, so any record whose fp64 best IoU lies within
1e-4 of 0.3, 0.5 or 0.7 has f[2], f[3] redrawn (test_loss_gpu.py's method and margin), and inputs() then asserts the condition
and iou_loss_cases' tie margin again.  No record is left out of any comparison."""
import ctypes
import math

import numpy as np
import torch

from conftest import COCO_ANCHORS
import test_loss_gpu as TL
import iou_loss_cases as IC

# ---- assignment -----------------------------------------------------------------------------------------------------------
DARKNET_THRESH = 0.213
# (w, h): (best anchor, extras above 0.213), anchors numbered 0..8 smallest first
HAND = {(40, 50): (3, {1, 2, 4, 5}), (12, 14): (0, {1, 2}), (300, 280): (8, {7}), (60, 80): (5, {3, 4, 6})}
STRIDE_OF = lambda k: (8, 16, 32)[k // 3]


def box(cx, cy, w, h, mix=1.0):
    return [cx - w / 2., cy - h / 2., cx + w / 2., cy + h / 2., mix]


def host(boxes, labels, img_size, class_num, thresh):
    from yolov3_tensorflow_amd.utils import data_utils
    return data_utils.process_box_host(boxes, labels, img_size, class_num, COCO_ANCHORS, thresh)


def records(ys):
    """{(anchor 0..8, gx, gy): ((cx, cy, w, h), [class bits set], mix weight)} of the object records of one image's y_true"""
    out = {}
    for s, y in enumerate(ys):
        for gy, gx, slot in np.argwhere(y[..., 4] != 0):
            r = y[gy, gx, slot]
            assert r[4] == 1.
            out[((2 - s) * 3 + int(slot), int(gx), int(gy))] = (tuple(float(v) for v in r[:4]),
                                                                np.flatnonzero(r[5:-1]).tolist(), float(r[-1]))
    return out


def expected_records(cx, cy, w, h, anchors_hit, bits, mix=1.0):
    f = np.float32
    geo = (float((f(cx - w / 2.) + f(cx + w / 2.)) / f(2)), float((f(cy - h / 2.) + f(cy + h / 2.)) / f(2)),
           float(f(cx + w / 2.) - f(cx - w / 2.)), float(f(cy + h / 2.) - f(cy - h / 2.)))
    return {(k, int(geo[0] // STRIDE_OF(k)), int(geo[1] // STRIDE_OF(k))): (geo, sorted(bits), mix) for k in anchors_hit}


def collision_case():
    """A 40 x 50 box (class 0) followed by a 60 x 80 box (class 2) with the same centre, in a 416 x 416 image.  The census,
    asserted here: both boxes hit anchor 3 (best of the first, an extra of the second) in the same 26-grid cell."""
    boxes = np.array([box(200., 180., 40, 50, 0.5), box(200., 180., 60, 80, 0.25)], np.float32)
    labels = np.array([0, 2])
    alone = [records(host(boxes[i:i + 1], labels[i:i + 1], [416, 416], 3, DARKNET_THRESH)) for i in range(2)]
    cell = (3, 200 // 16, 180 // 16)
    assert cell in alone[0] and cell in alone[1]
    assert {k for k, _, _ in alone[0]} == {3} | HAND[(40, 50)][1] and {k for k, _, _ in alone[1]} == {5} | HAND[(60, 80)][1]
    return boxes, labels, cell


GPU_W, GPU_H, GPU_C, GPU_KMAX, GPU_COUNTS = 96, 64, 3, 6, (6, 0, 3)


def gpu_case():
    """n = 3, image 96 x 64 (W x H), 3 classes, kmax 6, counts (6, 0, 3): (boxes [3,6,5], labels [3,6], counts).  Image 0: the
    three hand sizes, the collision pair, and a label outside [0, 3).  Image 1: no box (its rows hold boxes that must not be
    read).  Image 2: a centre left of the image (cx = -4: truncation instead of floor would put it into column 0), a label
    of -1, a box in the last cell; its rows behind the count hold boxes that must not be read."""
    b = np.zeros((3, GPU_KMAX, 5), np.float32)
    l = np.zeros((3, GPU_KMAX), np.int32)
    b[0] = [box(20., 30., 40, 50), box(70., 10., 12, 14, 0.75), box(50., 40., 300, 280, 0.5), box(60., 44., 40, 50, 0.3),
            box(60., 44., 60, 80, 0.6), box(90., 60., 33, 23)]
    l[0] = [0, 1, 2, 0, 2, 7]
    b[1] = [box(10. + 12 * i, 8. + 9 * i, 30, 61) for i in range(GPU_KMAX)]
    l[1] = 1
    b[2] = [box(-4., 30., 40, 50), box(40., 40., 16, 30, 0.9), box(95.5, 63.5, 12, 14), box(30., 20., 62, 45),
            box(50., 50., 116, 90), box(70., 20., 10, 13)]
    l[2] = [1, -1, 2, 0, 1, 2]
    return b, l, np.array(GPU_COUNTS, np.int32)


def host_batch(boxes, labels, counts, img_size, class_num, thresh):
    """process_box_host image by image -> three arrays [n, gh, gw, 3, 6 + C]"""
    per = [host(boxes[i, :counts[i]], labels[i, :counts[i]], img_size, class_num, thresh) for i in range(len(counts))]
    return [np.stack([p[s] for p in per]) for s in range(3)]


def device_assign(boxes, labels, counts, img_size, class_num, thresh, poison=None, entry='y3_process_box_multi'):
    """One call of the C entry: three device tensors (pre-filled with `poison` when given) and the status"""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    n, kmax = boxes.shape[:2]
    W, H = img_size
    bt, lt = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev), torch.from_numpy(labels.astype(np.int32)).to(dev)
    ct = torch.from_numpy(np.asarray(counts, np.int32)).to(dev)
    ys = [torch.empty((n, H // s, W // s, 3, 6 + class_num), device=dev) for s in (32, 16, 8)]
    if poison is not None:
        for y in ys:
            y.fill_(poison)
    anc = np.ascontiguousarray(COCO_ANCHORS, np.float32)
    ancp = anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    if entry == 'y3_process_box':
        rc = L.y3_process_box(fw.context(), fw.ptr(bt), fw.ptr(lt), fw.ptr(ct), n, kmax, class_num, W, H, ancp,
                              fw.ptr(ys[0]), fw.ptr(ys[1]), fw.ptr(ys[2]))
    else:
        rc = L.y3_process_box_multi(fw.context(), fw.ptr(bt), fw.ptr(lt), fw.ptr(ct), n, kmax, class_num, W, H, ancp,
                                    ctypes.c_float(thresh), fw.ptr(ys[0]), fw.ptr(ys[1]), fw.ptr(ys[2]))
    torch.cuda.synchronize()
    return rc, [y.cpu().numpy() for y in ys]


# ---- the conf rule's oracle -----------------------------------------------------------------------------------------------
THRESHOLDS = (0.3, 0.5, 0.7)
RULES = ((0.7, 0.0), (0.5, 1.0), (0.3, 0.5))        # (ignore_thresh, obj_iou_ratio) of the parity tests
KINDS = {'mse': 0, 'giou': 1, 'diou': 2, 'ciou': 3}
CASE_NAMES = IC.CASE_NAMES
MODES = IC.MODES

_INPUTS, _REFS = {}, {}


def objectness_target(pred, y_true, ratio):
    """z [..., 1]: (1 - r) + r * q where the record holds an object, q the plain IoU (box_iou) of its decoded prediction with
    its own true box - detached, NaN / inf / negative counted as 0 -, and 0 (selected) where it holds none"""
    q = IC.box_parts(pred.detach(), y_true[..., 0:4])['iou']
    q = torch.where(torch.isfinite(q) & (q >= 0), q, torch.zeros_like(q))
    m = y_true[..., 4]
    return torch.where(m != 0, (1. - ratio) + ratio * q, torch.zeros_like(q)).unsqueeze(-1)


def _graph_class():
    from oracle import train_ref
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    class ConfGraph(IC._graph_class()):
        def loss_layer(self, fm, y_true, anchors, use_label_smooth=False, use_focal_loss=False, box_loss='mse',
                       ignore_thresh=0.5, obj_iou_ratio=0.0):
            N, gh, gw = fm.shape[0], fm.shape[1], fm.shape[2]
            y_true = torch.as_tensor(np.asarray(y_true), dtype=self.dtype)
            anchors_t = torch.tensor(np.asarray(anchors, np.float32), dtype=self.dtype)
            ratio = torch.tensor([self.img_size[0] / gh, self.img_size[1] / gw], dtype=torch.float32).to(self.dtype)
            rr = torch.stack([ratio[1], ratio[0]])
            offset, pred_raw, conf_logits, prob_logits = self.reorg(fm, anchors)
            object_mask = y_true[..., 4:5]
            ignore = []
            for n in range(N):
                valid = y_true[n, ..., 0:4][object_mask[n, ..., 0] > 0.5]
                if valid.shape[0] == 0:
                    ignore.append(torch.ones(gh, gw, 3, dtype=self.dtype))          # the maximum over no box is -inf
                    continue
                best = train_ref.TrainGraph.box_iou(pred_raw[n].detach(), valid).max(dim=-1).values
                ignore.append((best < ignore_thresh).to(self.dtype))
            ignore_mask = torch.stack(ignore).unsqueeze(-1)
            pred_boxes = self.decode(fm, y_true, anchors)        # f[0:4] of the records without an object selected away
            mix_w = y_true[..., -1:]
            if box_loss == 'mse':
                true_xy = y_true[..., 0:2] / rr - offset
                pred_xy = pred_boxes[..., 0:2] / rr - offset
                true_twth = y_true[..., 2:4] / anchors_t
                pred_twth = pred_boxes[..., 2:4] / anchors_t
                true_twth = torch.where(true_twth == 0, torch.ones_like(true_twth), true_twth)
                pred_twth = torch.where(pred_twth == 0, torch.ones_like(pred_twth), pred_twth)
                true_twth = torch.log(torch.clamp(true_twth, 1e-9, 1e9))
                pred_twth = torch.log(torch.clamp(pred_twth, 1e-9, 1e9))
                scale = 2. - (y_true[..., 2:3] / float(self.img_size[1])) * (y_true[..., 3:4] / float(self.img_size[0]))
                xy_loss = torch.sum((true_xy - pred_xy) ** 2 * object_mask * scale * mix_w) / N
                wh_loss = torch.sum((true_twth - pred_twth) ** 2 * object_mask * scale * mix_w) / N
            else:
                xy_loss = IC.box_term(box_loss, pred_boxes, y_true, self.img_size, N)
                wh_loss = torch.zeros((), dtype=self.dtype)
            z = objectness_target(pred_raw, y_true, obj_iou_ratio)
            conf_pos = object_mask * bce(conf_logits, z, reduction='none')
            conf_neg = (1 - object_mask) * ignore_mask * bce(conf_logits, z, reduction='none')
            conf_loss = conf_pos + conf_neg
            if use_focal_loss:
                conf_loss = conf_loss * 1.0 * torch.abs(z - torch.sigmoid(conf_logits)) ** 2.0
            conf_loss = torch.sum(conf_loss * mix_w) / N
            target = y_true[..., 5:-1]
            if use_label_smooth:
                target = (1 - 0.01) * target + 0.01 * 1. / self.class_num
            class_loss = torch.sum(object_mask * bce(prob_logits, target, reduction='none') * mix_w) / N
            return xy_loss, wh_loss, conf_loss, class_loss
    return ConfGraph


def graph_for(class_num, img_hw, dtype=torch.float64):
    g = _graph_class()({}, class_num, dtype)
    g.img_size = list(img_hw)
    return g


def graph(case, dtype=torch.float64):
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    return graph_for(C, [H, W], dtype)


def near_a_threshold(best):
    return np.any([np.abs(best - t) < TL.IOU_MARGIN for t in THRESHOLDS], axis=0)


def inputs(case):
    """(logits [n, gh, gw, 3F] fp32, y_true fp32) of a case: iou_loss_cases' inputs, conditioned for every threshold"""
    if case in _INPUTS:
        return _INPUTS[case]
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    F = 5 + C
    fm0, y = IC.inputs(case)
    fm = fm0.copy().reshape(n, gh, gw, 3, F)
    flat = lambda: fm.reshape(n, gh, gw, 3 * F)
    pinned = (np.abs(fm[..., 2:4]) >= 25.).any(-1)          # the saturated and the overflowing records stay as they are
    rng = np.random.RandomState(3000 + seed)
    if case == 'many_boxes':
        # Random logits leave only some 60 of the 3072 records of image 0 above 0.7.  150 records WITHOUT an object - the ones
        # the mask acts on - are made to predict the true box of an object record of their own cell (its centre lies in that
        # cell), shrunk to 0.9 of its width and height: IoU 0.81 with that box, and 5 % of its size (>= 0.3 px) between each
        # corner pair.
        anc = np.asarray(TL._anchors(scale), np.float64)
        logit = lambda p: np.log(p / (1 - p))
        made = 0
        for gy, gx, k in np.argwhere((y[0, ..., 4] == 0) & ~pinned[0]):
            sib = np.flatnonzero(y[0, gy, gx, :, 4] != 0)
            if made == 150 or not len(sib):
                continue
            t = y[0, gy, gx, sib[0], 0:4].astype(np.float64)
            fx, fy = t[0] / (W / gw) - gx, t[1] / (H / gh) - gy
            if not (0.02 < fx < 0.98 and 0.02 < fy < 0.98):
                continue
            fm[0, gy, gx, k, 0:4] = [logit(fx), logit(fy), math.log(0.9 * t[2] / anc[k][0]), math.log(0.9 * t[3] / anc[k][1])]
            made += 1
        assert made == 150
    for _ in range(20):
        close = near_a_threshold(TL.best_iou64(case, flat(), y))
        ties = IC.tie_violations(case, flat(), y)
        if not close.any() and not ties.any():
            break
        assert not (pinned & (close | ties)).any(), 'a pinned record sits at a threshold or a tie'
        fm[close, 2:4] = (rng.standard_normal((int(close.sum()), 2)) * 1.5).astype(np.float32)
        fm[ties & ~close, 0:4] = (rng.standard_normal((int((ties & ~close).sum()), 4)) * 1.5).astype(np.float32)
    best = TL.best_iou64(case, flat(), y)
    assert not near_a_threshold(best).any() and not IC.tie_violations(case, flat(), y).any()
    if case == 'many_boxes':                  # every mask must be decided by records on both sides of its threshold
        non = y[0, ..., 4] == 0               # (counted among the records without an object: a stronger condition)
        for t in THRESHOLDS:
            assert ((best[0] >= t) & non).sum() > 100 and ((best[0] < t) & non).sum() > 100, (t, int(((best[0] >= t) & non).sum()))
    if case == '5x7_c20':                     # the saturated object records are still there
        obj = np.argwhere(y[..., 4] != 0)
        assert fm[tuple(obj[0])][2] == 25. and fm[tuple(obj[1])][3] == -25.
    _INPUTS[case] = (flat().copy(), y)
    return _INPUTS[case]


def evaluate(case, kind, smooth, focal, ignore_thresh, obj_iou_ratio, dtype=torch.float64, data=None):
    """([xy or box, wh, conf, class], d(sum)/d(logits)) of a case in `dtype`"""
    fm, y = inputs(case) if data is None else data
    t = torch.tensor(fm, dtype=dtype, requires_grad=True)
    parts = graph(case, dtype).loss_layer(t, y, TL._anchors(TL.CASES[case][6]), smooth, focal, kind, ignore_thresh, obj_iou_ratio)
    sum(parts).backward()
    return [float(p.detach()) for p in parts], t.grad.numpy()


def reference(case, kind, smooth, focal, ignore_thresh, obj_iou_ratio):
    """the fp64 evaluation, computed once per key and left unchanged"""
    key = (case, kind, smooth, focal, ignore_thresh, obj_iou_ratio)
    if key not in _REFS:
        _REFS[key] = evaluate(case, kind, smooth, focal, ignore_thresh, obj_iou_ratio)
    return _REFS[key]


def check_gates(loss4, grad, want4, wantg, what=''):
    """the project's loss gates (test_loss_gpu.py): each term within 1e-4 |ref| + 1e-6, the gradient within 2e-4 of the
    tensor's max magnitude; the figures are printed first"""
    err = TL.rel_err(np.asarray(grad, np.float64), wantg)
    print('%s: loss %s (ref %s), grad rel err %.2e' % (what, [float(v) for v in loss4], want4, err))
    for name, a, b in zip(('xy', 'wh', 'conf', 'class'), loss4, want4):
        assert abs(float(a) - b) <= 1e-4 * abs(b) + 1e-6, (what, name, float(a), b)
    assert err < 2e-4, (what, err)


def run_conf(case, kind, smooth, focal, ignore_thresh, obj_iou_ratio, grad_stride, accumulate=0, loss4=None, entry='conf',
             data=None):
    """One y3_loss_layer_conf (or, entry='box', y3_loss_layer_box) call: grad pre-filled with NaN, the scratch with 0xFF.
    Returns (status, loss4, grad) on the host."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, dev = _lib.lib(), fw.default_device()
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    fm, y = inputs(case) if data is None else data
    fmg, yg = torch.from_numpy(fm).to(dev), torch.from_numpy(y).to(dev)
    grad = torch.full((n, gh, gw, grad_stride), float('nan'), device=dev)
    loss4 = torch.full((4,), float('nan'), device=dev) if loss4 is None else loss4.to(dev)
    scratch = torch.full((L.y3_loss_scratch_bytes(n, gh, gw),), 0xFF, dtype=torch.uint8, device=dev)
    anc = np.ascontiguousarray(TL._anchors(scale), np.float32)
    head = (fw.context(), fw.ptr(fmg), fw.ptr(yg), n, gh, gw, C, H, W, anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            int(smooth), int(focal), KINDS[kind])
    tail = (accumulate, fw.ptr(loss4), fw.ptr(grad), grad_stride, fw.ptr(scratch), ctypes.c_size_t(scratch.numel()))
    if entry == 'box':
        rc = L.y3_loss_layer_box(*(head + tail))
    else:
        rc = L.y3_loss_layer_conf(*(head + (ctypes.c_float(ignore_thresh), ctypes.c_float(obj_iou_ratio)) + tail))
    torch.cuda.synchronize()
    return rc, loss4.cpu(), grad.cpu()


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  The entry
# points of this feature are added from here, as iou_loss_cases.py, ema_cases.py, mosaic_cases.py and affine_cases.py add
# theirs: this module is imported whenever the suite is collected (tests/test_assign_cpu.py imports it).
# tests/test_assign_gpu.py and tests/test_conf_rule_gpu.py run the entries through that module's own test.
def _register_guard_band_entries():
    import test_guard_bands_gpu as TG
    if 'y3_net_train_set_conf_rule' in TG.EXCLUDED:
        return
    TG.EXCLUDED['y3_net_train_set_conf_rule'] = 'net handle'

    def process_box_multi(g, thresh):
        """the 96 x 64 call of test_assign_gpu.py: bit-exact against process_box_host"""
        boxes, labels, counts = gpu_case()
        n = len(counts)
        ancp = TG.host_f32(COCO_ANCHORS)
        specs = [TG.IN('boxes', boxes), TG.IN('labels', labels), TG.IN('counts', counts)] + [
            TG.OUT('y_true_%d' % s, (n, GPU_H // s, GPU_W // s, 3, 6 + GPU_C)) for s in (32, 16, 8)]

        def call(a):
            t = lambda k: TG.P(a[k])
            g('y3_process_box_multi', g.ctx, t('boxes'), t('labels'), t('counts'), n, GPU_KMAX, GPU_C, GPU_W, GPU_H, ancp,
              ctypes.c_float(thresh), t('y_true_32'), t('y_true_16'), t('y_true_8'))

        def verify(o):
            for s, want in zip((32, 16, 8), host_batch(boxes, labels, counts, [GPU_W, GPU_H], GPU_C, thresh)):
                np.testing.assert_array_equal(o['y_true_%d' % s].numpy(), want)
        return TG.run_of(specs, call, ['y_true_32', 'y_true_16', 'y_true_8'], verify)

    def loss_layer_conf(g, case, kind, smooth, focal, thresh, ratio):
        """a tight gradient stride (no pad lane): the gates of test_conf_rule_gpu.py"""
        n, gh, gw, H, W, Cn, scale, seed = TL.CASES[case]
        fm, y = inputs(case)
        want4, wantg = reference(case, kind, smooth, focal, thresh, ratio)
        lanes = 3 * (5 + Cn)
        sb = g.L.y3_loss_scratch_bytes(n, gh, gw)
        ancp = TG.host_f32(TL._anchors(scale))
        specs = [TG.IN('feature_map', fm), TG.IN('y_true', y), TG.OUT('loss4', (4,)), TG.OUT('grad', (n, gh, gw, lanes)),
                 TG.S('scratch', sb)]

        def call(a):
            P = TG.P
            g('y3_loss_layer_conf', g.ctx, P(a['feature_map']), P(a['y_true']), n, gh, gw, Cn, H, W, ancp, int(smooth),
              int(focal), KINDS[kind], ctypes.c_float(thresh), ctypes.c_float(ratio), 0, P(a['loss4']), P(a['grad']), lanes,
              P(a['scratch']), ctypes.c_size_t(sb))

        def verify(o):
            gnp = o['grad'].numpy()
            assert np.isfinite(gnp).all()
            check_gates(o['loss4'].tolist(), gnp, want4, wantg, 'guarded %s' % case)
        return TG.run_of(specs, call, ['loss4', 'grad'], verify)

    TG.entry('process_box_multi-96x64-c3-t0.213', ('y3_process_box_multi',), process_box_multi, DARKNET_THRESH)
    TG.entry('loss_layer_conf-5x7_c20-ciou-tight', ('y3_loss_layer_conf',), loss_layer_conf, '5x7_c20', 'ciou', True, True, 0.7, 1.0)
    # (ema_cases.py: when this module is imported before pytest has read test_guard_bands' parametrize mark, whose list of ids
    # was made when that module was imported, the new entries need their ids there; imported later, nothing changes)
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entries()
