"""Cases and the fp64 oracle of the IoU box losses (include/yolo355.h at y3_loss_layer_box), shared by test_iou_loss_cpu.py,
test_iou_loss_gpu.py and test_iou_loss_train_gpu.py.

The oracle: box_x / box_term copy the header's formulas literally in torch (alpha detached), on the boxes the oracle's own
reorg decodes; IouGraph.loss_layer puts that term beside the conf and class terms of oracle.train_ref.TrainGraph.loss_layer
and returns (box term, 0, conf, class).  The gradient is autograd's.

The cases are test_loss_gpu.py's (CASES, inputs, anchors by import; its cached arrays are copied, never changed), plus:
  * two records WITHOUT an object get f[2] = 90 and f[3] = -90 (exp overflows / underflows in fp32) in every case;
  * many_boxes gets one object record whose predicted box is disjoint from its true box (inter == 0: the IoU's gradient
    vanishes, only the enclosing term pulls) and one whose predicted box encloses the true one, forced by logits;
  * 5x7_c20 keeps test_loss_gpu.py's saturated object records (f[2] = 25, f[3] = -25).
build() asserts that the set holds each of these.

Conditioning.  The derivative of a min / max jumps at a tie; an fp32 / fp64 disagreement about the side would move that record's
gradient by O(1).  fp32 coordinates at 608 px are good to 608 * 2^-24 = 4e-5 px, so every object record keeps 1e-3 px (more
than 10x that) between each corner pair (p1x / t1x, p2x / t2x, the same in y) and between each intersection edge and 0, in
fp64 (tie_violations has the one exemption, a predicted box thinner than the margin itself): a record that does not has its
f[0:4] redrawn, and build() then asserts the condition.  The ignore mask's own margin
(test_loss_gpu.py: no best IoU within 1e-4 of 0.5) is asserted again on the records it acts on, those without an object.  No
record is ever left out of a comparison."""
import math

import numpy as np
import torch

import test_loss_gpu as TL

KINDS = {'giou': 1, 'diou': 2, 'ciou': 3}
CASE_NAMES = ('1x2_c1', '5x7_c20', '5x7_r30x32', '20x28_c3', 'many_boxes')
MODES = ((False, False), (True, True))
TIE_MARGIN = 1e-3

_INPUTS, _REFS = {}, {}


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def box_parts(p, t):
    """the header's intermediate quantities of predicted boxes p [..., 4] and true boxes t [..., 4] (cx, cy, w, h)"""
    px, py, pw, ph = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    tx, ty, tw, th = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    p1x, p2x, p1y, p2y = px - pw / 2, px + pw / 2, py - ph / 2, py + ph / 2
    t1x, t2x, t1y, t2y = tx - tw / 2, tx + tw / 2, ty - th / 2, ty + th / 2
    ex = torch.minimum(p2x, t2x) - torch.maximum(p1x, t1x)
    ey = torch.minimum(p2y, t2y) - torch.maximum(p1y, t1y)
    inter = torch.clamp(ex, min=0) * torch.clamp(ey, min=0)
    union = pw * ph + tw * th - inter + 1e-10
    cw = torch.maximum(p2x, t2x) - torch.minimum(p1x, t1x)
    ch = torch.maximum(p2y, t2y) - torch.minimum(p1y, t1y)
    return dict(inter=inter, union=union, iou=inter / union, cw=cw, ch=ch, ex=ex, ey=ey,
                corners=torch.stack([p1x - t1x, p2x - t2x, p1y - t1y, p2y - t2y], -1))


def box_x(kind, p, t):
    """GIoU / DIoU / CIoU of p with t, as include/yolo355.h writes them"""
    q = box_parts(p, t)
    iou, cw, ch, union = q['iou'], q['cw'], q['ch'], q['union']
    if kind == 'giou':
        return iou - (cw * ch - union) / (cw * ch + 1e-10)
    diou = iou - ((p[..., 0] - t[..., 0]) ** 2 + (p[..., 1] - t[..., 1]) ** 2) / (cw ** 2 + ch ** 2 + 1e-10)
    if kind == 'diou':
        return diou
    assert kind == 'ciou', kind
    v = (4 / math.pi ** 2) * (torch.atan(t[..., 2] / t[..., 3]) - torch.atan(p[..., 2] / p[..., 3])) ** 2
    alpha = (v / (1 - iou + v + 1e-10)).detach()
    return diou - alpha * v


def box_term(kind, pred, y_true, img_hw, n):
    """sum (1 - X) * m * (2 - (tw / img_w)(th / img_h)) * mixup_weight / N.  Selected on m: a record without an object
    contributes exactly 0."""
    m = y_true[..., 4]
    scale = 2. - (y_true[..., 2] / float(img_hw[1])) * (y_true[..., 3] / float(img_hw[0]))
    x = box_x(kind, pred, y_true[..., 0:4])
    return torch.where(m != 0, (1 - x) * m * scale * y_true[..., -1], torch.zeros_like(x)).sum() / n


def _graph_class():
    from oracle import train_ref

    class IouGraph(train_ref.TrainGraph):
        def decode(self, fm, y_true, anchors):
            """the oracle's reorg on fm with f[0:4] of the records without an object replaced by 0: they are selected away
            BEFORE the decode, as the header asks (their exp may be inf), so they get an exactly zero box gradient"""
            n, gh, gw, _ = fm.shape
            f = fm.reshape(n, gh, gw, 3, 5 + self.class_num)
            obj = (y_true[..., 4:5] != 0)
            f = torch.cat([torch.where(obj, f[..., 0:4], torch.zeros_like(f[..., 0:4])), f[..., 4:]], -1)
            return self.reorg(f.reshape(n, gh, gw, -1), anchors)[1]

        def loss_layer(self, fm, y_true, anchors, use_label_smooth=False, use_focal_loss=False, box_loss='giou'):
            _, _, conf, cls = super(IouGraph, self).loss_layer(fm, y_true, anchors, use_label_smooth, use_focal_loss)
            yt = torch.as_tensor(np.asarray(y_true), dtype=self.dtype)
            box = box_term(box_loss, self.decode(fm, yt, anchors), yt, self.img_size, fm.shape[0])
            return box, torch.zeros((), dtype=self.dtype), conf, cls
    return IouGraph


def graph(case, dtype=torch.float64):
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    g = _graph_class()({}, C, dtype)
    g.img_size = [H, W]
    return g


def graph_for(class_num, img_hw, dtype=torch.float64):
    g = _graph_class()({}, class_num, dtype)
    g.img_size = list(img_hw)
    return g


def evaluate(case, kind, smooth, focal, dtype=torch.float64):
    """([box, 0, conf, class], d(sum)/d(logits)) of a case in `dtype`"""
    fm, y = inputs(case)
    t = torch.tensor(fm, dtype=dtype, requires_grad=True)
    parts = graph(case, dtype).loss_layer(t, y, TL._anchors(TL.CASES[case][6]), smooth, focal, kind)
    sum(parts).backward()
    return [float(p.detach()) for p in parts], t.grad.numpy()


def reference(case, kind, smooth, focal):
    """the fp64 evaluation, computed once per (case, kind, mode) and left unchanged"""
    key = (case, kind, smooth, focal)
    if key not in _REFS:
        _REFS[key] = evaluate(case, kind, smooth, focal)
    return _REFS[key]


# ---- the cases ------------------------------------------------------------------------------------------------------------
def parts64(case, fm, y):
    """box_parts in fp64 for every record of a case ([n, gh, gw, 3] each)"""
    yt = torch.tensor(y, dtype=torch.float64)
    pred = graph(case).decode(torch.tensor(fm, dtype=torch.float64), yt, TL._anchors(TL.CASES[case][6]))
    out = {k: v.numpy() for k, v in box_parts(pred, yt[..., 0:4]).items()}
    out.update(pw=pred[..., 2].numpy(), ph=pred[..., 3].numpy())
    return out


def tie_violations(case, fm, y):
    """object records with a corner pair or an intersection edge within TIE_MARGIN of a tie"""
    q = parts64(case, fm, y)
    near = (np.abs(q['corners']) < TIE_MARGIN).any(-1)
    # (an edge of the intersection cannot be longer than the predicted box: where that box is itself thinner than the margin
    # - the saturated f[3] = -25 record, ph = 1e-9 px - the edge is exempt.  Its side of the clamp reaches the gradient only
    # through d inter / d ph, which the decode multiplies by d ph / d f3 = ph: a disagreement there moves that lane by < 1e-3
    # of its unsaturated size, not by O(1).  The record's corner pairs are held to the margin like everyone's.)
    near |= (np.abs(q['ex']) < TIE_MARGIN) & (q['pw'] >= TIE_MARGIN)
    near |= (np.abs(q['ey']) < TIE_MARGIN) & (q['ph'] >= TIE_MARGIN)
    return near & (y[..., 4] != 0)


def inputs(case):
    """(logits [n, gh, gw, 3F] fp32, y_true [n, gh, gw, 3, 6+C] fp32) of a case, built once on the CPU"""
    if case in _INPUTS:
        return _INPUTS[case]
    n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
    F = 5 + C
    fm0, y = TL.inputs(case)
    fm = fm0.copy().reshape(n, gh, gw, 3, F)
    anc = np.asarray(TL._anchors(scale), np.float64)
    obj = np.argwhere(y[..., 4] != 0)
    non = np.argwhere(y[..., 4] == 0)
    # exp(f) that overflows / underflows, on two records without an object
    r_over, r_under = tuple(non[0]), tuple(non[1])
    fm[r_over][2] = 90.
    fm[r_under][3] = -90.
    forced = []
    if case == 'many_boxes':
        # the two object records with the narrowest true boxes (6 .. 7 px on a stride of 8)
        order = np.argsort(y[..., 2][tuple(obj.T)])
        r_dis, r_enc = tuple(obj[order[0]]), tuple(obj[order[1]])
        # disjoint: a predicted box of a hundredth of the anchor, its centre at the cell's edge farther from the true centre
        tx_in_cell = y[r_dis][0] / (W / gw) - r_dis[2]
        fm[r_dis][0:4] = [-12. if tx_in_cell > 0.5 else 12., 0.3, math.log(0.01), math.log(0.012)]
        # enclosing: a predicted box of three times the true one around the cell's centre
        k = r_enc[3]
        fm[r_enc][0:4] = [0.1, -0.2, math.log(3 * y[r_enc][2] / anc[k][0]), math.log(3.5 * y[r_enc][3] / anc[k][1])]
        forced = [r_dis, r_enc]
    rng = np.random.RandomState(2000 + seed)
    flat = lambda: fm.reshape(n, gh, gw, 3 * F)
    for _ in range(20):
        bad = tie_violations(case, flat(), y)
        if not bad.any():
            break
        assert not any(bad[r] for r in forced), 'a forced record sits at a tie'
        fm[bad, 0:4] = (rng.standard_normal((int(bad.sum()), 4)) * 1.5).astype(np.float32)
    assert not tie_violations(case, flat(), y).any()
    # the ignore mask's margin, on the records the mask acts on
    best = TL.best_iou64(case, flat(), y)
    assert not ((np.abs(best - 0.5) < TL.IOU_MARGIN) & (y[..., 4] == 0)).any()
    if case == '5x7_c20':              # test_loss_gpu.py's saturated object records are still there
        r0, r1 = tuple(obj[0]), tuple(obj[1])
        assert fm[r0][2] == 25. and fm[r1][3] == -25.
    assert fm[r_over][2] == 90. and fm[r_under][3] == -90. and y[r_over][4] == 0 and y[r_under][4] == 0
    _INPUTS[case] = (flat().copy(), y)
    return _INPUTS[case]


def build():
    """every case's inputs, and the assertion that the set holds what the tests are about (the inputs do not depend on the
    kind, so neither does this census): {what: number of object records}"""
    census = dict(disjoint=0, pred_encloses_true=0, true_encloses_pred=0, saturated=0, overflow_non_object=0, objects=0)
    for case in CASE_NAMES:
        fm, y = inputs(case)
        n, gh, gw, H, W, C, scale, seed = TL.CASES[case]
        m = y[..., 4] != 0
        q = parts64(case, fm, y)
        c = q['corners']
        census['objects'] += int(m.sum())
        census['disjoint'] += int(((q['inter'] == 0) & m).sum())
        census['pred_encloses_true'] += int(((c[..., 0] < 0) & (c[..., 1] > 0) & (c[..., 2] < 0) & (c[..., 3] > 0) & m).sum())
        census['true_encloses_pred'] += int(((c[..., 0] > 0) & (c[..., 1] < 0) & (c[..., 2] > 0) & (c[..., 3] < 0) & m).sum())
        f = fm.reshape(n, gh, gw, 3, 5 + C)
        census['saturated'] += int((((f[..., 2] == 25.) | (f[..., 3] == -25.)) & m).sum())
        census['overflow_non_object'] += int((((f[..., 2] == 90.) | (f[..., 3] == -90.)) & ~m).sum())
    assert census['disjoint'] >= 1 and census['pred_encloses_true'] >= 1, census
    assert census['saturated'] >= 2 and census['overflow_non_object'] == 2 * len(CASE_NAMES), census
    return census


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  The two entry
# points of the IoU losses are added to that table from here: this module is imported whenever the suite is collected.
def _register_guard_band_entries():
    import ctypes
    import test_guard_bands_gpu as TG
    if 'y3_net_train_set_box_loss' in TG.EXCLUDED:
        return
    TG.EXCLUDED['y3_net_train_set_box_loss'] = 'net handle'

    def loss_layer_box(g, case, kind, smooth, focal):
        """5x7_c20 with a tight gradient stride (no pad lane): the gates of test_iou_loss_gpu.py"""
        n, gh, gw, H, W, Cn, scale, seed = TL.CASES[case]
        fm, y = inputs(case)
        want4, wantg = reference(case, kind, smooth, focal)
        lanes = 3 * (5 + Cn)
        sb = g.L.y3_loss_scratch_bytes(n, gh, gw)
        ancp = TG.host_f32(TL._anchors(scale))
        specs = [TG.IN('feature_map', fm), TG.IN('y_true', y), TG.OUT('loss4', (4,)), TG.OUT('grad', (n, gh, gw, lanes)),
                 TG.S('scratch', sb)]

        def call(a):
            P = TG.P
            g('y3_loss_layer_box', g.ctx, P(a['feature_map']), P(a['y_true']), n, gh, gw, Cn, H, W, ancp, int(smooth), int(focal),
              KINDS[kind], 0, P(a['loss4']), P(a['grad']), lanes, P(a['scratch']), ctypes.c_size_t(sb))

        def verify(o):
            for name, a, b in zip(('box', 'wh', 'conf', 'class'), o['loss4'].tolist(), want4):
                assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (name, a, b)
            gnp = o['grad'].numpy()
            assert np.isfinite(gnp).all() and TL.rel_err(gnp, wantg) < 2e-4
        return TG.run_of(specs, call, ['loss4', 'grad'], verify)

    TG.entry('loss_layer_box-5x7_c20-ciou-tight', ('y3_loss_layer_box',), loss_layer_box, '5x7_c20', 'ciou', True, True)


_register_guard_band_entries()
