"""GPU tests of the bf16-storage path (BASELINE configs[4]).  Per-op: the bf16 conv against an fp64 convolution
of the SAME bf16-rounded operands — the only differences are the fp32 accumulation order and the single final
rounding, so the bound is one bf16 ulp (2^-8 relative) plus fp32 accumulation noise.  Whole network (416 and the
configs[4] size 608): gated against the fp32 oracle at 3 % max / 2 % rms of the logits (bf16 is not held to the 1e-3
box tolerance)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import blob_images

pytestmark = pytest.mark.gpu


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def ref_conv(x, w_hwio, scale, shift, k, stride, act, resid=None):
    xd = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wd = torch.from_numpy(w_hwio).double().permute(3, 2, 0, 1)
    if stride > 1:
        y = F.conv2d(F.pad(xd, (1, 1, 1, 1)), wd, stride=stride)
    else:
        y = F.conv2d(xd, wd, padding=k // 2)
    y = y * torch.from_numpy(scale).double().view(1, -1, 1, 1) + torch.from_numpy(shift).double().view(1, -1, 1, 1)
    if act:
        y = torch.where(y > 0, y, 0.1 * y)
    y = y.permute(0, 2, 3, 1)
    if resid is not None:
        y = y + torch.from_numpy(resid).double()
    return y.numpy()


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout,resid,c_up,out_f32', [
    (3, 20, 28, 3, 1, 128, 256, True, 0, 0), (2, 26, 26, 3, 2, 64, 128, False, 0, 0),
    (3, 20, 28, 1, 1, 256, 128, False, 0, 0), (2, 26, 26, 1, 1, 768, 256, False, 256, 0),
    (2, 19, 19, 1, 1, 1024, 255, False, 0, 1), (3, 20, 28, 3, 1, 32, 64, True, 0, 0),
    (2, 24, 24, 1, 1, 64, 32, False, 0, 0), (1, 13, 13, 3, 1, 512, 1024, False, 0, 0),
    # the LDS-DMA kernel's tile shapes (y3_conv_bf16x.hip): 256x256 / 256x128 tiles need > 448 tiles, so larger maps;
    # stride 2 with Cin = 32 (64-byte rows), a ragged last row block, a 1x1 with Cout = 64, fused upsample with 128+256
    (4, 76, 76, 3, 1, 128, 256, True, 0, 0), (8, 76, 76, 3, 1, 256, 512, False, 0, 0),
    (2, 38, 50, 3, 2, 32, 64, False, 0, 0), (1, 37, 41, 3, 1, 64, 128, True, 0, 0),
    (3, 20, 28, 1, 1, 128, 64, False, 0, 0), (2, 26, 26, 1, 1, 384, 128, False, 128, 0),
    # round 5, the 192-row tiles of the pipelined 3x3 kernel (y3_conv_bf16x.hip: 38-grid bs=16 -> 192x256, 19-grid -> 192x128)
    (16, 38, 38, 3, 1, 256, 512, True, 0, 0), (16, 19, 19, 3, 1, 512, 1024, False, 0, 0), (5, 38, 38, 3, 2, 128, 256, False, 0, 0),
    # round 5, the persistent ring kernel of the 1x1 convs (y3_conv_bf16r.hip): many tiles per workgroup with one and two
    # K-steps per tile (the ring runs across tile boundaries), ragged rows, a Cout that is no multiple of 32, a residual,
    # bf16 output with Cout % 8 != 0 (per-element epilogue), fp32 output with a residual, deep K
    (4, 152, 152, 1, 1, 64, 32, False, 0, 0), (8, 152, 152, 1, 1, 128, 64, False, 0, 0), (16, 76, 76, 1, 1, 256, 128, False, 0, 0),
    (3, 21, 27, 1, 1, 192, 136, True, 0, 0), (2, 38, 38, 1, 1, 512, 256, True, 0, 0), (1, 19, 19, 1, 1, 1024, 512, False, 0, 0),
    (2, 13, 17, 1, 1, 128, 100, False, 0, 0), (2, 13, 17, 1, 1, 128, 255, True, 0, 1), (16, 76, 76, 1, 1, 256, 255, False, 0, 1),
    (4, 38, 38, 1, 1, 768, 256, False, 256, 0),
    # the /32 and /16 layers of a 32 x 64 input (maps 1x2 and 2x4: a 3x3 conv on a map one pixel high, whose top and bottom
    # taps read only padding); the per-op twins of tests/test_bf16_plan_gpu.py's (1,32,64) step
    (1, 1, 2, 3, 1, 512, 1024, False, 0, 0), (2, 1, 2, 1, 1, 1024, 512, False, 0, 0), (1, 2, 4, 1, 1, 768, 256, False, 256, 0),
])
def test_bf16_conv_matches_fp64_on_rounded_operands(n, h, w, k, stride, cin, cout, resid, c_up, out_f32):
    from yolov3_tensorflow_amd import framework as fw, _lib
    dev = fw.default_device()
    L, ctx = _lib.lib(), fw.context()
    rng = np.random.RandomState(cin * 7 + cout)
    cx = cin - c_up
    x = bf16_round(rng.standard_normal((n, h, w, cx)))
    xu = bf16_round(rng.standard_normal((n, h // 2, w // 2, c_up))) if c_up else None
    wt = bf16_round(rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin)))
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(0, 0.2, cout).astype(np.float32)
    r = bf16_round(rng.standard_normal((n, h // stride, w // stride, cout))) if resid else None
    xin = x if xu is None else np.concatenate([np.repeat(np.repeat(xu, 2, 1), 2, 2), x], axis=3)
    want = ref_conv(xin, wt, scale, shift, k, stride, not out_f32, r)
    tb = lambda a: None if a is None else torch.from_numpy(a).to(dev).to(torch.bfloat16).contiguous()
    wg = torch.from_numpy(wt).to(dev)
    wp = torch.empty(k * k * cout * cin, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_pack_conv_weights_bf16(ctx, fw.ptr(wg), k, cin, cout, fw.ptr(wp)))
    y = torch.empty((n, h // stride, w // stride, cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    d = _lib.ConvDesc(n, h, w, cin, c_up, cout, k, stride, 0 if out_f32 else 1)
    xg, xug, rg = tb(x), tb(xu), tb(r)                     # keep the device buffers alive across the launch
    scg, shg = torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)
    _lib.check(L.y3_conv2d_fwd_bf16(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(xug), fw.ptr(wp), fw.ptr(scg),
                                    fw.ptr(shg), fw.ptr(rg), fw.ptr(y), out_f32))
    got = y.float().cpu().numpy()
    tol = (1e-4 if out_f32 else 2.0 ** -8) * np.abs(want) + 2e-3
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= tol).all(), float(np.abs(got - want).max())


@pytest.mark.parametrize('n,h,w', [(2, 64, 96), (1, 70, 38), (3, 32, 32), (1, 608, 608)])
def test_bf16_fused_stem_and_stride2_conv(n, h, w):
    """The stem and the stride-2 conv behind it in one kernel (y3_conv2d_fwd_bf16_stem_s2, csrc/y3_conv_bf16s.hip) against
    fp64 convolutions of the same bf16-rounded operands, the stem's output rounded to bf16 in between as the kernel does
    (utils/layer_utils.py:34-40).  Maps that are no multiple of the 16 x 16 tile, several images, the bench's own size.  A
    stem value that sits on a bf16 rounding boundary may round the other way (fp32 against fp64 accumulation): one bf16 ulp
    of one input of the second conv, covered by the absolute term."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    dev = fw.default_device()
    L, ctx = _lib.lib(), fw.context()
    rng = np.random.RandomState(h * 7 + w)
    x = bf16_round(rng.uniform(0, 1, (n, h, w, 3)))
    w0 = bf16_round(rng.standard_normal((3, 3, 3, 32)) * np.sqrt(2.0 / 27))
    w1 = bf16_round(rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / 288))
    sc0, sh0 = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.normal(0, 0.2, 32).astype(np.float32)
    sc1, sh1 = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
    mid = bf16_round(ref_conv(x, w0, sc0, sh0, 3, 1, True))
    want = ref_conv(mid, w1, sc1, sh1, 3, 2, True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w1p = torch.empty(9 * 64 * 32, dtype=torch.bfloat16, device=dev)
    w1g = t(w1)
    _lib.check(L.y3_pack_conv_weights_bf16(ctx, fw.ptr(w1g), 3, 32, 64, fw.ptr(w1p)))
    y = torch.empty((n, h // 2, w // 2, 64), dtype=torch.bfloat16, device=dev)
    xg, w0g, a0, b0, a1, b1 = t(x), t(w0), t(sc0), t(sh0), t(sc1), t(sh1)
    _lib.check(L.y3_conv2d_fwd_bf16_stem_s2(ctx, n, h, w, fw.ptr(xg), fw.ptr(w0g), fw.ptr(a0), fw.ptr(b0), fw.ptr(w1p),
                                            fw.ptr(a1), fw.ptr(b1), fw.ptr(y)))
    got = y.float().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    tol = 2.0 ** -7 * np.abs(want) + 2e-2
    assert (err <= tol).all(), (float(err.max()), float(np.abs(want).max()))
    print('fused stem + stride-2 conv %dx%dx%d: max |d| %.3e (max |ref| %.2f), mean |d| %.3e' % (n, h, w, err.max(), np.abs(want).max(), err.mean()))


@pytest.mark.parametrize('n,h,w', [(2, 32, 48), (1, 35, 19), (3, 16, 16), (1, 304, 304)])
def test_bf16_fused_first_residual_block(n, h, w):
    """res_block(net, 32) on a 64-channel map as one kernel (y3_resblock64_fwd_bf16, csrc/y3_conv_bf16b.hip) against fp64
    convolutions of the same bf16-rounded operands, the 32-channel tensor rounded to bf16 in between as the kernel does
    (utils/layer_utils.py:25-32).  Maps that are no multiple of the 16 x 16 tile, several images, the bench's own size."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    dev = fw.default_device()
    L, ctx = _lib.lib(), fw.context()
    rng = np.random.RandomState(h * 5 + w)
    x = bf16_round(rng.standard_normal((n, h, w, 64)))
    w2 = bf16_round(rng.standard_normal((1, 1, 64, 32)) * np.sqrt(2.0 / 64))
    w3 = bf16_round(rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / 288))
    sc2, sh2 = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.normal(0, 0.2, 32).astype(np.float32)
    sc3, sh3 = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
    mid = bf16_round(ref_conv(x, w2, sc2, sh2, 1, 1, True))
    want = ref_conv(mid, w3, sc3, sh3, 3, 1, True, x)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w2g, w3g = t(w2), t(w3)
    w2p = torch.empty(64 * 32, dtype=torch.bfloat16, device=dev)
    w3p = torch.empty(9 * 64 * 32, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_pack_conv_weights_bf16(ctx, fw.ptr(w2g), 1, 64, 32, fw.ptr(w2p)))
    _lib.check(L.y3_pack_conv_weights_bf16(ctx, fw.ptr(w3g), 3, 32, 64, fw.ptr(w3p)))
    xg = t(x).to(torch.bfloat16).contiguous()
    y = torch.empty((n, h, w, 64), dtype=torch.bfloat16, device=dev)
    a2, b2, a3, b3 = t(sc2), t(sh2), t(sc3), t(sh3)
    _lib.check(L.y3_resblock64_fwd_bf16(ctx, n, h, w, fw.ptr(xg), fw.ptr(w2p), fw.ptr(a2), fw.ptr(b2), fw.ptr(w3p),
                                        fw.ptr(a3), fw.ptr(b3), fw.ptr(y)))
    got = y.float().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    tol = 2.0 ** -7 * np.abs(want) + 2e-2
    assert (err <= tol).all(), (float(err.max()), float(np.abs(want).max()))
    print('fused residual block %dx%dx%d: max |d| %.3e (max |ref| %.2f), mean |d| %.3e' % (n, h, w, err.max(), np.abs(want).max(), err.mean()))


@pytest.mark.parametrize('size', [416, 608])
def test_bf16_forward_tracks_the_fp32_oracle(gpu_model, size):
    """configs[4] (608x608 bf16 storage) and the 416 size: the deviation from the fp32 oracle is GATED, not just
    reported — max |d| <= 3 % of the largest logit, rms <= 2 % (measured: 1.6 % / 1.2 %: 75 layers of bf16 rounding at
    2^-9 relative each); bf16 is not held to the 1e-3 box tolerance of the fp32 path."""
    import yolov3_tensorflow_amd as y3
    from oracle import yolo_ref
    model, params = gpu_model
    x = blob_images(0, 2 if size == 416 else 1, size)
    ref = yolo_ref.forward(params, x)
    model.compute_dtype = 'bf16'
    try:
        with y3.variable_scope('yolov3'):
            fms = model.forward(x, False)
            again = model.forward(x, False)
    finally:
        model.compute_dtype = 'f32'
    for i, (g, g2, r) in enumerate(zip(fms, again, ref)):
        assert g.dtype == torch.float32 and torch.equal(g, g2)
        g = g.cpu().numpy()
        rel = float(np.abs(g - r).max() / np.abs(r).max())
        rms = float(np.sqrt(((g - r) ** 2).mean()) / np.sqrt((r ** 2).mean()))
        print('bf16 feature_map_%d: max err / max|ref| = %.3e, rms rel = %.3e' % (i + 1, rel, rms))
        assert np.isfinite(g).all() and rel < 0.03 and rms < 0.02
    # fp32 path is untouched by the excursion
    with y3.variable_scope('yolov3'):
        f32 = model.forward(x, False)
    assert np.abs(f32[0].cpu().numpy() - ref[0]).max() < 2e-4


def test_configs4_bs16_608_boxes_scores_and_nms_track_the_fp32_oracle(gpu_model, anchors):
    """BASELINE configs[4] at its own size (608x608, bs=16, bf16 storage): beyond the feature-map gate, the DECODED
    outputs and the detections (ref: model.py:140-190, utils/nms_utils.py:8-48) against the fp32 CPU oracle on all 16
    images.  bf16 storage is not a 1e-3 path; the gates below follow from the feature-map gate (|d logit| <= 3 % of the
    largest logit ~ 0.4: d sigmoid <= 0.25 * 0.4, d exp relative <= e^0.4 - 1) and are stated, the measured values are
    printed:
      * feature maps: max |d| <= 3 % of max |ref|, rms <= 2 % (all 16 images, every scale);
      * confs / probs: max |d| <= 0.11, mean |d| <= 0.01;
      * box corners: |d| <= 4 px + 0.6 * box scale for every box, median |d| / box scale <= 2 %;
      * per-class NMS at ~150 candidates per image (score threshold = a quantile of the oracle's scores), IoU 0.45:
        >= 80 % of the oracle's detections have a same-class GPU detection with IoU >= 0.7 (mean over the batch), and
        the GPU's own selection is bit-exact against the C NMS oracle on the GPU's decoded tensors."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd.utils import nms_utils
    from oracle import yolo_ref, nms_ref
    model, params = gpu_model
    n, size = 16, 608
    x = blob_images(5, n, size)
    torch.set_num_threads(min(torch.get_num_threads(), 64))
    ref = [np.concatenate(p) for p in zip(*[yolo_ref.forward(params, x[i:i + 4]) for i in range(0, n, 4)])]
    model.compute_dtype = 'bf16'
    try:
        with y3.variable_scope('yolov3'):
            fms = model.forward(x, False)
            again = model.forward(x, False)
            boxes, confs, probs, scores = model.predict(fms, with_scores=True)
    finally:
        model.compute_dtype = 'f32'
    for i, (g, g2, r) in enumerate(zip(fms, again, ref)):
        assert torch.equal(g, g2), 'bs=16 bf16 forward is not run-to-run bit-exact'
        g = g.cpu().numpy()
        rel = float(np.abs(g - r).max() / np.abs(r).max())
        rms = float(np.sqrt(((g - r) ** 2).mean()) / np.sqrt((r ** 2).mean()))
        print('bs=16 @608 bf16 feature_map_%d: max err / max|ref| = %.3e, rms rel = %.3e' % (i + 1, rel, rms))
        assert np.isfinite(g).all() and rel < 0.03 and rms < 0.02
    rb, rc, rp = yolo_ref.predict(ref, anchors, [size, size], 80)
    gb, gc, gp, gs = (t.cpu().numpy() for t in (boxes, confs, probs, scores))
    dc, dp = np.abs(gc - rc), np.abs(gp - rp)
    print('bs=16 @608 bf16: confs max |d| %.3e mean %.3e; probs max |d| %.3e mean %.3e' % (dc.max(), dc.mean(), dp.max(), dp.mean()))
    assert dc.max() <= 0.11 and dp.max() <= 0.11 and dc.mean() <= 0.01 and dp.mean() <= 0.01
    scale = np.maximum(np.abs(rb[..., 2:] - rb[..., :2]).max(axis=-1, keepdims=True), 1.0)      # the box's larger side
    db = np.abs(gb - rb)
    print('bs=16 @608 bf16: box corners max |d| %.3f px, max |d|/side %.3e, median |d|/side %.3e'
          % (db.max(), (db / scale).max(), np.median((db / scale).max(axis=-1))))
    assert (db <= 4.0 + 0.6 * scale).all()
    assert np.median((db / scale).max(axis=-1)) <= 0.02
    # detections
    rs = rc * rp
    thr = float(np.quantile(rs, 1 - 150.0 / rs[0].size))
    out = nms_utils.gpu_nms_batched(boxes, scores, 80, 100, thr, 0.45, return_index=True)

    def iou(p, q):
        iw = min(p[2], q[2]) - max(p[0], q[0])
        ih = min(p[3], q[3]) - max(p[1], q[1])
        if iw <= 0 or ih <= 0:
            return 0.0
        return iw * ih / ((p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - iw * ih)

    fracs = []
    gt_dict, val_preds = {}, []        # the fp32 oracle's detections as ground truth, the bf16 path's as predictions
    for i in range(n):
        b, s, l, idx = (t.cpu().numpy() for t in out[i])
        ob, osc, ol, oi = nms_ref.c_per_class('tf', gb[i], gs[i], 80, 100, thr, 0.45)
        np.testing.assert_array_equal(idx, oi)                         # identical inputs: bit-exact selection
        np.testing.assert_array_equal(l, ol)
        eb, es, el, ei = nms_ref.c_per_class('tf', rb[i], rs[i], 80, 100, thr, 0.45)
        hit = sum(1 for k in range(len(el)) if any(l[j] == el[k] and iou(b[j], eb[k]) >= 0.7 for j in range(len(l))))
        fracs.append(hit / float(max(len(el), 1)))
        gt_dict[i] = [[float(v) for v in eb[k]] + [int(el[k])] for k in range(len(el))]
        val_preds += [[i] + [float(v) for v in b[j]] + [float(s[j]), int(l[j])] for j in range(len(l))]
    print('bs=16 @608 bf16: oracle detections recovered (same class, IoU >= 0.7): mean %.3f, worst image %.3f'
          % (float(np.mean(fracs)), float(np.min(fracs))))
    assert float(np.mean(fracs)) >= 0.8
    # The same comparison in the reference's own accuracy metric (eval.py:61-75, 125-140: VOC AP per class, mean over the classes;
    # utils/eval_utils.py:343-423 voc_eval): what storing activations and weights in bf16 costs in mAP when the fp32 path's
    # detections are taken as the truth.
    import contextlib
    import io
    from yolov3_tensorflow_amd.utils import eval_utils

    def voc_map(gt, preds, thres):
        aps = []
        with contextlib.redirect_stdout(io.StringIO()):
            for c in range(80):
                npos, nd, rec, prec, ap = eval_utils.voc_eval(gt, preds, c, iou_thres=thres)
                if npos >= 1:
                    aps.append(float(ap))
        return float(np.mean(aps)), len(aps)

    # (1) Context, printed and NOT gated (rounds 3-5 gated it): truth = the oracle's detections AT the score
    # threshold, predictions = the bf16 path's at the same threshold.  With synthetic weights ~150 detections per image sit at
    # that threshold and none is confident: which of them cross it is decided by last bits (0.81-0.86 / 0.79-0.84 measured at
    # EQUAL feature-map error, depending only on which kernels run the first layers) - this number cannot resolve a regression.
    for thres in (0.5, 0.75):
        m, nc = voc_map(gt_dict, val_preds, thres)
        print('bs=16 @608 bf16 (context, ungated): mAP@%.2f with truth and predictions cut at the same threshold (%d classes): %.3f'
              % (thres, nc, m))
    # (2) The gate: the same metric on a scene where it can resolve something - confident detections, and SCORE MARGINS around
    # the cut.  Scene: the same network with the objectness and class rows of its three detection convs scaled by k (a power of
    # two: the convs are linear, model.py:55-57, and a power-of-two scale commutes with every rounding of either path, so scaling
    # those channels of BOTH paths' feature maps is exactly that network); k = the smallest power of two at which the fp32
    # oracle has >= 30 detections per image scoring >= 0.5.  Levels: truth = the oracle's detections scoring >= 0.5 (greedy
    # NMS keeps the same high-scored boxes whatever the cut below them); predictions = the bf16 path's detections scoring >= 0.3;
    # the oracle's detections in the band [0.15, 0.5) are "difficult" in the VOC sense - a prediction that matches one of them
    # (same class, IoU >= the evaluation's) and no truth box is left out, neither hit nor false alarm.  A truth box is then lost
    # only when bf16 storage drags its score from >= 0.5 below 0.3 or its box below the IoU bar; a false alarm is a bf16
    # detection >= 0.3 whose fp32 counterpart scores < 0.15 or does not exist.  A real 10-point loss (a wrong layer, a missing
    # residual) cannot hide in it.
    def scaled(fm, k):
        v = fm.reshape(fm.shape[0], fm.shape[1], fm.shape[2], 3, 85).clone() if torch.is_tensor(fm) else \
            fm.reshape(fm.shape[0], fm.shape[1], fm.shape[2], 3, 85).copy()
        v[..., 4:] *= k
        return v.reshape(fm.shape)

    k = 1
    while k < 256:
        _, kc, kp = yolo_ref.predict([scaled(r, float(k)) for r in ref], anchors, [size, size], 80)
        if float(((kc * kp) >= 0.5).sum()) / n >= 30:
            break
        k *= 2
    assert k < 256, 'no power-of-two scale of the detection rows gives the oracle 30 confident candidates per image'
    rb2, rc2, rp2 = yolo_ref.predict([scaled(r, float(k)) for r in ref], anchors, [size, size], 80)
    rs2 = rc2 * rp2
    with y3.variable_scope('yolov3'):
        b2, c2, p2, s2 = model.predict([scaled(f, float(k)) for f in fms], with_scores=True)
    t_hi, t_mid, t_lo = 0.5, 0.3, 0.15
    out2 = nms_utils.gpu_nms_batched(b2, s2, 80, 100, t_mid, 0.45, return_index=True)
    gt_hi, band, preds2 = {}, {}, []
    for i in range(n):
        eb, es, el, ei = nms_ref.c_per_class('tf', rb2[i], rs2[i], 80, 100, t_lo, 0.45)
        gt_hi[i] = [[float(v) for v in eb[j]] + [int(el[j])] for j in range(len(el)) if es[j] >= t_hi]
        band[i] = [(eb[j], int(el[j])) for j in range(len(el)) if es[j] < t_hi]
        b, sc, l, idx = (t.cpu().numpy() for t in out2[i])
        preds2 += [[i] + [float(v) for v in b[j]] + [float(sc[j]), int(l[j])] for j in range(len(l))]
    n_truth = sum(len(v) for v in gt_hi.values())
    print('bs=16 @608 bf16: detection rows scaled by %d: %d confident oracle detections (>= 0.5) after NMS, %d bf16 detections >= 0.3'
          % (k, n_truth, len(preds2)))
    assert n_truth >= 16 * 10, 'too few confident oracle detections (%d) for the metric to mean anything' % n_truth
    # (measured in round 6: k = 1 - the synthetic logits already spread over +-6 -, 36,189 truth boxes on the 16 images, mAP@0.5
    # 0.982, mAP@0.75 0.936; VERDICT r5 asked for floors >= 0.85)
    for thres, floor in ((0.5, 0.95), (0.75, 0.90)):
        kept = []
        for pr in preds2:
            i, box, lab = pr[0], pr[1:5], pr[6]
            if any(g[4] == lab and iou(box, g[:4]) >= thres for g in gt_hi[i]):
                kept.append(pr)
            elif not any(bl == lab and iou(box, bb) >= thres for bb, bl in band[i]):
                kept.append(pr)
        m, nc = voc_map(gt_hi, kept, thres)
        print('bs=16 @608 bf16: mAP@%.2f against the fp32 oracle\'s confident detections (%d boxes; band [0.15, 0.5) difficult; '
              '%d of %d predictions evaluated; %d classes): %.3f' % (thres, n_truth, len(kept), len(preds2), nc, m))
        assert m >= floor
