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


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', [s for s in SHAPES if s[6] % 4 == 0])
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
    z = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=dev)
    st = torch.full((nb, 2, cout), float('nan'), device=dev)
    xg = x.to(dev)
    _lib.check(L.y3_conv2d_train_fwd_bf16(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(wp), fw.ptr(z), fw.ptr(st)))
    ref = conv_ref(x.double(), wb, k, stride)
    zc = z.double().cpu()
    e = within_one_rounding(zc, ref)
    # the partials are the sums of z AS STORED: against fp64 sums of the stored values
    s = st.double().cpu().sum(0)
    e_s = rel_err(s[0], zc.reshape(-1, cout).sum(0))
    e_q = rel_err(s[1], (zc.reshape(-1, cout) ** 2).sum(0))
    print('fwd %s: z %.2f roundings, partial sums %.1e / %.1e' % ((n, h, w, k, stride, cin, cout), e, e_s, e_q))
    assert e <= 2.05                       # one rounding (measured 1.97-1.99), plus the fp32 accumulation's noise
    assert e_s < 4e-7 and e_q < 4e-7      # measured: <= 1.3e-7 (fp32 sums of 128 rows per block, fp64 over blocks)


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', SHAPES)
@pytest.mark.parametrize('acc', [0, 1])
def test_dgrad_writes_and_accumulates(n, h, w, k, stride, cin, cout, acc):
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(cin + 7 * cout + k)
    dzs = ((cout + 31) // 32) * 32
    ho, wo = h // stride, w // stride
    dz = bf16_exact(rng, (n, ho, wo, cout))
    dzp = torch.zeros((n, ho, wo, dzs), dtype=torch.bfloat16)
    dzp[..., :cout] = dz
    wt = torch.tensor(rng.standard_normal((k, k, cin, cout)) * 0.1, dtype=torch.float32)
    wb = wt.to(torch.bfloat16).double()
    x = torch.zeros((n, h, w, cin), dtype=torch.float64, requires_grad=True)
    conv_ref(x, wb, k, stride).backward(dz.double())
    d = _lib.ConvDesc(n, h, w, cin, 0, cout, k, stride, 0)
    wp = torch.empty(k * k * dzs * cin, dtype=torch.bfloat16, device=dev)
    _lib.check(L.y3_pack_conv_weights_bf16_train(ctx, fw.ptr(wt.to(dev)), k, cin, cout, dzs, fw.ptr(wp)))
    prior = torch.tensor(rng.standard_normal((n, h, w, cin)), dtype=torch.float32)
    dx = prior.clone().to(dev) if acc else torch.full((n, h, w, cin), float('nan'), device=dev)
    _lib.check(L.y3_conv2d_dgrad_bf16(ctx, ctypes.byref(d), fw.ptr(dzp.to(dev)), dzs, fw.ptr(wp), acc, fw.ptr(dx)))
    want = x.grad + (prior.double() if acc else 0)
    e = rel_err(dx.cpu(), want)
    print('dgrad %s acc=%d: %.2e' % ((n, h, w, k, stride, cin, cout), acc, e))
    assert e < 1.2e-6                      # measured: <= 4.1e-7 (fp32 accumulation of bf16-exact products)


def _wgrad(fw, _lib, L, ctx, dev, x, dzp, k, stride, cout):
    n, h, w, cin = x.shape
    dzs = dzp.shape[-1]
    d = _lib.ConvDesc(n, h, w, cin, 0, cout, k, stride, 0)
    sb = L.y3_conv_wgrad_bf16_scratch_bytes(ctypes.byref(d))
    sc = torch.empty(max(sb, 16), dtype=torch.uint8, device=dev)
    dw = torch.full((k, k, cin, cout), float('nan'), device=dev)
    _lib.check(L.y3_conv_wgrad_bf16(ctx, ctypes.byref(d), fw.ptr(x), fw.ptr(dzp), dzs, fw.ptr(dw), fw.ptr(sc),
                                    ctypes.c_size_t(sb)))
    dw2 = torch.empty_like(dw)
    _lib.check(L.y3_conv_wgrad_bf16(ctx, ctypes.byref(d), fw.ptr(x), fw.ptr(dzp), dzs, fw.ptr(dw2), fw.ptr(sc),
                                    ctypes.c_size_t(sb)))
    assert torch.equal(dw, dw2)            # fixed summation order
    return dw


@pytest.mark.parametrize('n,h,w,k,stride,cin,cout', SHAPES)
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
    (43527, 12, 0), (600, 1028, 0)])
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
