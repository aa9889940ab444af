"""Each kernel of the bf16 train step (net dtype 1) on bf16-exact inputs against fp64 torch on the same rounded inputs.

What is left is fp32 accumulation order, plus - where the kernel's output is bf16 - the one rounding to nearest even at
the store.  bf16 outputs are therefore held element by element to one rounding to nearest of the fp64 value (at most half
a bf16 ulp: 2 in the units of within_one_rounding, measured 1.97-1.99); fp32 outputs to about 3x the measured max-abs
relative error (stated at each gate)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))


def within_one_rounding(got, want):
    """worst |got - want| / (2^-9 |want| + tiny): one rounding to nearest is at most half an ulp, <= 2 in these units"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (2.0 ** -9 * np.abs(want) + 1e-6 * np.abs(want).max() + 1e-30)).max())


def _env():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context(), fw.default_device()


def bf16_exact(rng, shape, scale=1.0):
    return torch.tensor(rng.standard_normal(shape) * scale, dtype=torch.float32).to(torch.bfloat16)


def conv_ref(x, w_hwio, k, stride):
    """fp64 conv of NHWC x with an HWIO kernel (SAME padding as the network: stride-2 pads 1 on each side)"""
    xp = x.permute(0, 3, 1, 2)
    wt = w_hwio.permute(3, 2, 0, 1)
    if stride > 1:
        z = F.conv2d(F.pad(xp, (1, 1, 1, 1)), wt, stride=stride)
    else:
        z = F.conv2d(xp, wt, padding=k // 2)
    return z.permute(0, 2, 3, 1)


# the shapes of test_train_gpu.py::test_conv_wgrad_and_dgrad_match_autograd (Cin = 3: the stem keeps its fp32 kernels)
SHAPES = [(2, 20, 28, 3, 1, 64, 128), (2, 20, 28, 1, 1, 128, 64), (3, 16, 24, 3, 2, 32, 64), (2, 13, 13, 1, 1, 256, 255),
          (2, 26, 26, 3, 1, 32, 64), (2, 12, 12, 3, 2, 128, 256),
          # the detection convs at 20 classes (VOC) and at one class: dz row stride 96 and 32, cout % 4 != 0
          (2, 13, 13, 1, 1, 256, 75), (2, 13, 13, 1, 1, 512, 18)]
MEASURED = {}

# The shapes the bf16 kernels' OWN code branches on (y3_conv_bf16.hip: conv_train_body, dispatch_t, y3_launch_conv_bf16_dgrad;
# y3_wgrad_bf16.hip: wgrad_bf16_kernel, plan_of).  Each line: the branch the case reaches; what it would catch.  M = output rows,
# S = K-steps of 32 channels, BN = the column tile dispatch_t picks (32 / 64 / 128 for Cout <= 32 / <= 64 / above).
FWD_SHAPES = [s for s in SHAPES if s[6] % 4 == 0] + [
    # launch_t<32,4,1,..,EPI=1> (C4 = 8, RPP = 32, two passes, the 32-way column-sum combine), the 1x1 64 -> 32 of the first
    # residual block; would catch: a wrong rows-per-pass or combine stride that only BN = 32 has
    (2, 20, 28, 1, 1, 64, 32),
    # Cout = 20 below BN = 32, 3x3: `co < p.Cout`, `r0 < BN` and `cok` false inside the live tile; would catch: weight rows or
    # partial columns past Cout read or written (the NaN-filled partials keep no room for a stray store)
    (1, 10, 14, 3, 1, 32, 20),
    # ragged BN = 64 tile (Cout = 36) on an odd 13x13 map, M = 338: two full row blocks and one of 82 rows; would catch: a
    # partial row or a z row written with the tile's width, not Cout's
    (2, 13, 13, 1, 1, 128, 36),
    # odd map under a 3x3 stride-1 conv, second 128-column block half empty (Cout = 192); would catch: a border mask that is
    # right only where the row length divides the tile, columns 128.. taken from block 0
    (2, 13, 13, 3, 1, 64, 192),
    # stride 2 onto an odd 13x13 output grid (26 -> 13, the network's 38 -> 19 in small); would catch: oy, ox decoded with the
    # input's width, or the left/top pad applied on the wrong side
    (2, 26, 26, 3, 2, 64, 128),
    # S = 144 K-steps, the network's deepest reduction (3x3 512 -> 1024 at 13x13): 9 taps x 16 channel chunks through the
    # two-ahead loader; would catch: a tap / chunk wrap that drifts only after many steps.  4608 terms per output: z measured
    # 1.98 roundings, so the 2.05 gate holds as it is, with no accumulation term
    (1, 13, 13, 3, 1, 512, 1024),
    # S = 1 (1x1, Cin = 32), M = 60 below one row tile: the prologue issues past the end, the loop body runs once and
    # compute(1) is skipped; would catch: the unconsumed second K-step added in, rows 60.. counted in the partials
    (1, 6, 10, 1, 1, 32, 64),
]
DGRAD_SHAPES = SHAPES + [
    # stride 2, odd 13x13 dz grid, forward Cin = 64: the BN = 64 TMODE instantiation; would catch: a parity class that
    # assumes an even grid (the last dz row / column dropped or wrapped into the next image)
    (2, 26, 26, 3, 2, 64, 128),
    # non-square odd 5x13 dz grid, dz_stride 96: S = 3, 6, 6, 12 over the four classes, so the one-tap class has an odd S
    # (the `g + 1 < S` guard, the clamped wtap); would catch: Ho and Wo swapped, the look-ahead K-step of a clamped tap summed
    (1, 10, 26, 3, 2, 32, 96),
    # ragged output column block: forward Cin = 192, above 128 and no multiple of it, odd map; would catch: columns 128..191
    # written from the wrong weight rows, or a store past column 191
    (2, 13, 13, 3, 1, 192, 64),
    # reduction of 9 * 1024 (S = 288), 512 output columns: the deepest data gradient of the network
    (1, 13, 13, 3, 1, 512, 1024),
    # S = 1: 1x1 with dz_stride 32, the gradient of layer 2; would catch: what the forward S = 1 case does, in EPI = 2
    (2, 20, 28, 1, 1, 64, 32),
]
# fp32 accumulation over 9216 terms, eight times the deepest reduction the 1.2e-6 gate was measured on (1152 terms: 4.1e-7):
# measured 1.74e-6 (acc = 0) and 1.72e-6 (acc = 1) against the fp64 gradient of the same rounded operands; about 3x that.
# (The expected order: 576 MFMA accumulations onto a sum of magnitude 16-32, each rounding uniform in +-2^-20, walk to
# sqrt(576) * 0.55e-6 = 1.3e-5 rms and to 6e-5 at the 4.4-sigma worst of 86,528 outputs; over max|dx| of about 4.3 standard
# deviations of sqrt(9216) * 0.1, i.e. about 41: 1.4e-6.)
DGRAD_GATE = {(1, 13, 13, 3, 1, 512, 1024): 5.2e-6}
WGRAD_SHAPES = SHAPES + [
    # J = k*k*Cin = 64 below the 128-row tile, Cout = 32: `jok` false for half the staging threads, three quarters of the dz
    # columns past dz_stride; would catch: P columns 64.. staged from x instead of zero
    (2, 20, 28, 1, 1, 64, 32),
    # J = 32, M = 60: one split of two K-steps, the second with 28 live rows; would catch: rows past M multiplied in
    (1, 6, 10, 1, 1, 32, 64),
    # odd map, 3x3: the tap's border pixels are zero rows of P; would catch: iy / ix decoded with the wrong width.  Its 11
    # K-steps go to two splits of 6 and 5 (pinned below): a short last split of several steps
    (2, 13, 13, 3, 1, 64, 192),
    # odd stride-2 output grid (13x13 from 26x26); would catch: the pad applied to the wrong side under stride 2
    (2, 26, 26, 3, 2, 64, 128),
    # 2050 rows = 65 K-steps, one output tile: nine splits of 8 K-steps, the ninth with ONE K-step of two live rows (`more`
    # false on the first trip); would catch: a last split that reads a K-step it never loaded, or skips its only one
    (2, 25, 41, 1, 1, 128, 64),
]
# plan_of, by hand: ns = min(ceil(1024 / tiles), (ksteps + 7) / 8), chunk = ceil(ksteps / ns), nsplit = ceil(ksteps / chunk).
#   (2,25,41,1,1,128,64): ksteps 65, tiles 1 -> ns 9, chunk 8, nsplit 9 (8 x 8 + 1)
#   (2,13,13,3,1,64,192): ksteps 11, tiles 5 x 2 -> ns 2, chunk 6, nsplit 2 (6 + 5; the last K-step has 18 rows)
#   (1,6,10,1,1,32,64):   ksteps 2 -> one split (no scratch)
# Pinned so that a changed plan fails here instead of silently moving the case off its branch.
WGRAD_SPLITS = {(2, 25, 41, 1, 1, 128, 64): 9, (2, 13, 13, 3, 1, 64, 192): 2, (1, 6, 10, 1, 1, 32, 64): 1}


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', FWD_SHAPES)
def test_train_forward_z_and_its_column_partials(n, h, w, k, stride, cin, cout):
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(cin + cout + k)
    x = bf16_exact(rng, (n, h, w, cin))
    wt = torch.tensor(rng.standard_normal((k, k, cin, cout)) * 0.1, dtype=torch.float32)
    wb = wt.to(torch.bfloat16).double()                       # the packing rounds the kernel once
    d = _lib.ConvDesc(n, h, w, cin, 0, cout, k, stride, 0)
    wp = torch.empty(k * k * cin * cout, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_pack_conv_weights_bf16_train(ctx, fw.ptr(wt.to(dev)), k, cin, cout, 0, fw.ptr(wp)))
    ho, wo = h // stride, w // stride
    nb = L.y3_conv_train_stats_blocks_bf16(ctypes.byref(d))
    assert nb == (n * ho * wo + 127) // 128
    z = torch.full((n, ho, wo, cout), float('nan'), dtype=torch.bfloat16, device=dev)
    st = torch.full((nb, 2, cout), float('nan'), device=dev)
    xg = x.to(dev)
    _lib.check(L.y3_conv2d_train_fwd_bf16(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(wp), fw.ptr(z), fw.ptr(st)))
    ref = conv_ref(x.double(), wb, k, stride)
    zc = z.double().cpu()
    e = within_one_rounding(zc, ref)
    # the partials are the sums of z AS STORED: against fp64 sums of the stored values
    stc = st.double().cpu()
    s = stc.sum(0)
    zr = zc.reshape(-1, cout)
    e_s = rel_err(s[0], zr.sum(0))
    e_q = rel_err(s[1], (zr ** 2).sum(0))
    # ... and block by block: block b's two rows are the sums over rows [128 b, min(128 b + 128, M)) and nothing else, each
    # held against that block's own largest sum (would catch: a row counted in its neighbour's block, which the total hides)
    zb = torch.zeros((nb * 128, cout), dtype=torch.float64)
    zb[:zr.shape[0]] = zr
    zb = zb.reshape(nb, 128, cout)
    want_b = torch.stack([zb.sum(1), (zb ** 2).sum(1)], 1)                      # [nb][2][cout]
    e_b = float(((stc - want_b).abs().amax(2) / want_b.abs().amax(2).clamp_min(1e-12)).max())
    print('fwd %s: z %.2f roundings, partial sums %.1e / %.1e, worst block %.1e' % ((n, h, w, k, stride, cin, cout), e, e_s,
                                                                                   e_q, e_b))
    assert e <= 2.05                       # one rounding (measured 1.97-1.99), plus the fp32 accumulation's noise
    assert e_s < 4e-7 and e_q < 4e-7      # measured: <= 1.3e-7 (fp32 sums of 128 rows per block, fp64 over blocks)
    assert e_b < 4e-7                      # measured: <= 2.6e-7 (one block's fp32 sums); an unwritten partial is NaN: fails


_DGRAD_CASE = {}


def _dgrad_case(n, h, w, k, stride, cin, cout):
    """the operands of a data-gradient case and its fp64 gradient, computed once for acc = 0 and 1 and left unchanged"""
    key = (n, h, w, k, stride, cin, cout)
    if key not in _DGRAD_CASE:
        rng = np.random.RandomState(cin + 7 * cout + k)
        dz = bf16_exact(rng, (n, h // stride, w // stride, cout))
        wt = torch.tensor(rng.standard_normal((k, k, cin, cout)) * 0.1, dtype=torch.float32)
        wb = wt.to(torch.bfloat16).double()
        x = torch.zeros((n, h, w, cin), dtype=torch.float64, requires_grad=True)
        conv_ref(x, wb, k, stride).backward(dz.double())
        prior = torch.tensor(rng.standard_normal((n, h, w, cin)), dtype=torch.float32)
        _DGRAD_CASE[key] = (dz, wt, x.grad.detach(), prior)     # (a few hundred thousand values in all)
    return _DGRAD_CASE[key]


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', DGRAD_SHAPES)
@pytest.mark.parametrize('acc', [0, 1])
def test_dgrad_writes_and_accumulates(n, h, w, k, stride, cin, cout, acc):
    fw, _lib, L, ctx, dev = _env()
    dzs = ((cout + 31) // 32) * 32
    ho, wo = h // stride, w // stride
    dz, wt, grad, prior = _dgrad_case(n, h, w, k, stride, cin, cout)
    dzp = torch.zeros((n, ho, wo, dzs), dtype=torch.bfloat16)
    dzp[..., :cout] = dz
    d = _lib.ConvDesc(n, h, w, cin, 0, cout, k, stride, 0)
    wp = torch.empty(k * k * dzs * cin, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_pack_conv_weights_bf16_train(ctx, fw.ptr(wt.to(dev)), k, cin, cout, dzs, fw.ptr(wp)))
    dx = prior.clone().to(dev) if acc else torch.full((n, h, w, cin), float('nan'), device=dev)
    _lib.check(L.y3_conv2d_dgrad_bf16(ctx, ctypes.byref(d), fw.ptr(dzp.to(dev)), dzs, fw.ptr(wp), acc, fw.ptr(dx)))
    want = grad + (prior.double() if acc else 0)
    e = rel_err(dx.cpu(), want)
    print('dgrad %s acc=%d: %.2e' % ((n, h, w, k, stride, cin, cout), acc, e))
    # measured: <= 4.1e-7 (fp32 accumulation of bf16-exact products)
    assert e < DGRAD_GATE.get((n, h, w, k, stride, cin, cout), 1.2e-6)


def _wgrad(fw, _lib, L, ctx, dev, x, dzp, k, stride, cout):
    n, h, w, cin = x.shape
    dzs = dzp.shape[-1]
    d = _lib.ConvDesc(n, h, w, cin, 0, cout, k, stride, 0)
    sb = L.y3_conv_wgrad_bf16_scratch_bytes(ctypes.byref(d))
    splits = WGRAD_SPLITS.get((n, h, w, k, stride, cin, cout))
    if splits is not None:                 # the case's split plan, pinned: a changed plan fails here
        assert sb == (splits * k * k * cin * cout * 4 if splits > 1 else 0), (sb, splits)
    sc = torch.empty(max(sb, 16), dtype=torch.uint8, device=dev)
    dw = torch.full((k, k, cin, cout), float('nan'), device=dev)
    _lib.check(L.y3_conv_wgrad_bf16(ctx, ctypes.byref(d), fw.ptr(x), fw.ptr(dzp), dzs, fw.ptr(dw), fw.ptr(sc),
                                    ctypes.c_size_t(sb)))
    dw2 = torch.empty_like(dw)
    _lib.check(L.y3_conv_wgrad_bf16(ctx, ctypes.byref(d), fw.ptr(x), fw.ptr(dzp), dzs, fw.ptr(dw2), fw.ptr(sc),
                                    ctypes.c_size_t(sb)))
    assert torch.equal(dw, dw2)            # fixed summation order
    return dw


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', WGRAD_SHAPES)
def test_wgrad(n, h, w, k, stride, cin, cout):
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(3 * cin + cout + k)
    dzs = ((cout + 31) // 32) * 32          # (255: the det_pad stride of the detection convs' dz)
    ho, wo = h // stride, w // stride
    x = bf16_exact(rng, (n, h, w, cin))
    dz = bf16_exact(rng, (n, ho, wo, cout))
    dzp = torch.zeros((n, ho, wo, dzs), dtype=torch.bfloat16)
    dzp[..., :cout] = dz
    wv = torch.zeros((k, k, cin, cout), dtype=torch.float64, requires_grad=True)
    conv_ref(x.double(), wv, k, stride).backward(dz.double())
    dw = _wgrad(fw, _lib, L, ctx, dev, x.to(dev), dzp.to(dev), k, stride, cout)
    e = rel_err(dw.cpu(), wv.grad)
    print('wgrad %s: %.2e' % ((n, h, w, k, stride, cin, cout), e))
    assert e < 5e-7                        # measured: <= 1.7e-7


def test_wgrad_on_a_concat_input():
    """the concat layers' weight gradient reads the materialised upsample+concat tensor (y3_upsample_concat_bf16, exact)"""
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(11)
    n, h, w, cu, cx, cout = 2, 26, 26, 128, 256, 128
    up, xr = bf16_exact(rng, (n, h // 2, w // 2, cu)), bf16_exact(rng, (n, h, w, cx))
    cat = torch.empty((n, h, w, cu + cx), dtype=torch.bfloat16, device=dev)
    upg, xg = up.to(dev), xr.to(dev)           # (held: a temporary's memory may be handed out again before the launch)
    _lib.check(L.y3_upsample_concat_bf16(ctx, fw.ptr(upg), cu, fw.ptr(xg), cx, n, h, w, fw.ptr(cat)))
    want = torch.cat([up.repeat_interleave(2, 1).repeat_interleave(2, 2), xr], -1)
    assert torch.equal(cat.cpu(), want)
    dz = bf16_exact(rng, (n, h, w, cout))
    wv = torch.zeros((1, 1, cu + cx, cout), dtype=torch.float64, requires_grad=True)
    conv_ref(want.double(), wv, 1, 1).backward(dz.double())
    dw = _wgrad(fw, _lib, L, ctx, dev, cat, dz.to(dev), 1, 1, cout)
    assert rel_err(dw.cpu(), wv.grad) < 5e-7


def test_wgrad_at_the_largest_rows_count():
    """bs=64 @416, layer 2 (1x1 64 -> 32 at 208x208): 2,768,896 rows over 1024 splits; fp64 reference on the device"""
    fw, _lib, L, ctx, dev = _env()
    g = torch.Generator(device=dev).manual_seed(5)
    n, h, w, cin, cout = 64, 208, 208, 64, 32
    x = torch.randn((n, h, w, cin), device=dev, generator=g).to(torch.bfloat16)
    dz = torch.randn((n, h, w, cout), device=dev, generator=g).to(torch.bfloat16)
    dw = _wgrad(fw, _lib, L, ctx, dev, x, dz, 1, 1, cout)
    want = x.reshape(-1, cin).double().t() @ dz.reshape(-1, cout).double()
    e = rel_err(dw.reshape(cin, cout).cpu(), want.cpu())
    print('wgrad at 2,768,896 rows: %.2e' % e)
    assert e < 4e-6                        # measured: 1.2e-6 (2.8 M products of unit-variance terms per output)


@pytest.mark.parametrize('rows,c,z_f32', [
    (2 * 13 * 13, 1024, 0), (3 * 20 * 28, 64, 0), (5000, 32, 1), (64, 256, 0),
    # the column reduction's other paths (tests/test_train_gpu.py::test_bn_train_forward_backward): 85 rows per pass with an
    # idle lane and a second trip of the row loop; two columns per thread, the second with one live lane
    (43527, 12, 0), (600, 1028, 0),
    # fewer rows than rows per pass (the fp32 list's case): every row lane past the third idle; would catch: an idle lane's
    # stale partial summed into the column
    (3, 256, 0)])
def test_bn_apply_and_backward(rows, c, z_f32):
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(rows + c)
    zb = torch.tensor(rng.standard_normal((rows, c)) * 2 + rng.standard_normal(c), dtype=torch.float32)
    if not z_f32:
        zb = zb.to(torch.bfloat16).float()
    z = zb.double().requires_grad_(True)
    gamma = torch.tensor(rng.uniform(0.5, 1.5, c), dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(rng.normal(0, 0.3, c), dtype=torch.float64, requires_grad=True)
    resid = bf16_exact(rng, (rows, c))
    mean, var = z.mean(0), z.var(0, unbiased=False)
    u = (z - mean) * gamma / torch.sqrt(var + 1e-5) + beta
    y = torch.where(u > 0, u, 0.1 * u)
    dy = torch.tensor(rng.standard_normal((rows, c)), dtype=torch.float32)
    y.backward(dy.double())
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)
    gg, bg = f32(gamma.detach()), f32(beta.detach())
    stats = torch.empty((4, c), device=dev)
    sc = torch.empty(L.y3_bn_bwd_scratch_bytes(c), dtype=torch.uint8, device=dev)
    _lib.check(L.y3_bn_train_stats(ctx, fw.ptr(f32(zb)), rows, c, fw.ptr(gg), fw.ptr(bg), ctypes.c_float(1e-5),
                                   ctypes.c_float(0.9), fw.ptr(stats[0]), fw.ptr(stats[1]), fw.ptr(stats[2]),
                                   fw.ptr(stats[3]), None, None, fw.ptr(sc)))
    zdev = f32(zb) if z_f32 else zb.to(torch.bfloat16).to(dev)
    yg = torch.empty((rows, c), dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_bn_apply_fwd_bf16(ctx, fw.ptr(zdev), z_f32, fw.ptr(stats[2]), fw.ptr(stats[3]), fw.ptr(resid.to(dev)),
                                      rows, c, fw.ptr(yg)))
    e_y = within_one_rounding(yg.double().cpu(), y.detach() + resid.double())
    assert e_y <= 2.05, e_y               # one rounding (measured 1.98-1.99)
    if z_f32:
        return                              # (the stem's BN backward is the fp32 one)
    dgam, dbet = torch.empty(c, device=dev), torch.empty(c, device=dev)
    dz = torch.empty((rows, c), dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_bn_train_bwd_bf16(ctx, fw.ptr(zdev), fw.ptr(f32(dy)), fw.ptr(gg), fw.ptr(stats[2]), fw.ptr(stats[3]),
                                      fw.ptr(stats[0]), fw.ptr(stats[1]), rows, c, fw.ptr(dgam), fw.ptr(dbet), fw.ptr(dz),
                                      fw.ptr(sc)))
    e_g, e_b = rel_err(dgam.cpu(), gamma.grad), rel_err(dbet.cpu(), beta.grad)
    e_z = within_one_rounding(dz.double().cpu(), z.grad)
    print('bn %d x %d: y %.2f roundings; dgamma %.1e dbeta %.1e; dz %.2f roundings' % (rows, c, e_y, e_g, e_b, e_z))
    # measured: <= 1.0e-7; 43527 x 12: 2.4e-7, 2.0e-7.  There a partial is a chain of up to 86 fp32 additions (two rows per
    # lane, then the 85 row lanes in order), and 512 such partials with independent roundings give an error of the order of
    # sqrt(512 * 86) * 2^-25 * |partial| / max|sum|, with |partial| ~ 11 and max|sum| ~ 3e2: 2e-7.  The inputs are seeded and the reduction has a fixed order (no
    # atomics), so the figure is the same bits on every run, not a sample.
    assert e_g < 3e-7 and e_b < 3e-7
    assert e_z <= 2.05                     # one rounding (measured 1.97-1.99)


def test_f32_to_bf16_rounds_to_nearest_even():
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(2)
    v = torch.tensor(rng.standard_normal(4096) * 10, dtype=torch.float32)
    v[:4] = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 0.0])     # ties
    out = torch.empty(4096, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_f32_to_bf16(ctx, fw.ptr(v.to(dev)), 4096, fw.ptr(out)))
    assert torch.equal(out.cpu(), v.to(torch.bfloat16))


@pytest.mark.parametrize('n,h,w,cu,cx', [
    # several images, an odd half-size map (3x5 -> 6x10), channel counts that are multiples of 4 but not of 8; would catch: yy/2,
    # xx/2 taken with the full map's width, an image stride of h*w for `up`, an 8-byte access assumed 16-byte aligned
    (3, 6, 10, 12, 20),
    # 1,056,768 quads against the 4096 x 256 = 1,048,576 threads grid_for's cap allows: the grid-stride loop's second trip;
    # would catch: a stride of the uncapped grid, i.e. the tail never written (the output starts as NaN)
    (2, 258, 256, 12, 20)])
def test_upsample_concat_is_an_exact_copy(n, h, w, cu, cx):
    fw, _lib, L, ctx, dev = _env()
    g = torch.Generator().manual_seed(n + h + w)
    # a copy moves any bit pattern: random 16-bit words, compared as words
    bits = lambda shape: (torch.randint(0, 2 ** 16, shape, generator=g, dtype=torch.int32) - 2 ** 15).to(torch.int16)
    up, xr = bits((n, h // 2, w // 2, cu)), bits((n, h, w, cx))
    cat = torch.full((n, h, w, cu + cx), float('nan'), dtype=torch.bfloat16, device=dev)
    upg, xg = up.to(dev), xr.to(dev)
    _lib.check(L.y3_upsample_concat_bf16(ctx, fw.ptr(upg), cu, fw.ptr(xg), cx, n, h, w, fw.ptr(cat)))
    want = torch.cat([up.repeat_interleave(2, 1).repeat_interleave(2, 2), xr], -1)
    assert torch.equal(cat.cpu().view(torch.int16), want)


def _f32(patterns):
    return torch.tensor(patterns, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_f32_to_bf16_at_the_ends_of_the_format():
    """+-0, +-Inf, the largest finite values, fp32 denormals: bit-equal to torch's conversion.  NaNs of any payload: a NaN.
    Would catch: integer rounding alone (u += 0x7FFF + lsb; u >> 16), whose increment carries out of a NaN's mantissa when its
    upper seven bits are all zero or all one: 0x7F800001 -> +Inf, 0x7FFFFFFF -> -0.0, 0xFFFFFFFF -> +0.0."""
    fw, _lib, L, ctx, dev = _env()
    to_i32 = lambda p: p - (1 << 32) if p >= (1 << 31) else p
    finite = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
              0x7F7FFFFF, 0xFF7FFFFF,                       # the largest finite float: rounds to +-Inf
              0x7F7F7FFF, 0x7F7F8000, 0x7F7E8000,           # just below the tie: stays finite; the ties: to Inf, to even
              0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x807FFFFF, 0x007F0000,   # denormals
              0x00010000,                                   # (a denormal that bf16 holds exactly)
              0x00800000, 0x3F800000, 0x3F808000, 0x3F818000, 0xBF808001, 0x3F7FFFFF]      # (the last: up into the next binade)
    nans = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F808000, 0xFF80FFFF, 0x7FFF8000]
    assert len(finite + nans) % 4 == 0
    v = _f32([to_i32(p) for p in finite + nans])
    assert bool(torch.isnan(v[len(finite):]).all()) and not bool(torch.isnan(v[:len(finite)]).any())
    out = torch.full((v.numel(),), 1.0, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_f32_to_bf16(ctx, fw.ptr(v.to(dev)), v.numel(), fw.ptr(out)))
    got = out.cpu()
    want = v.to(torch.bfloat16)
    print('f32 -> bf16:', ' '.join('%08x>%04x' % (p, b & 0xFFFF) for p, b in zip(finite + nans, got.view(torch.int16).tolist())))
    nf = len(finite)
    assert torch.equal(got[:nf].view(torch.int16), want[:nf].view(torch.int16))      # (bits: -0.0 == 0.0 as values)
    assert bool(torch.isnan(got[nf:]).all()), got[nf:]
