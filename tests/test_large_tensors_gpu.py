"""GPU, at true size: n = 64 at 512 x 512, the smallest batch-64 scale of the multi-scale schedule whose stem output (= layer
1's input and dy: 64 * 512^2 * 32 = 2^29 elements) the fp32 conv launchers used to refuse.  They now run it as two launches
of 32 images.

Per-pixel outputs: images 0, 31 | 32 (either side of the one range boundary) and 63 against an fp64 CPU conv at the
tolerance tests/test_conv_gpu.py holds that kernel to (1e-4 + 1e-4 |ref|; the data gradient: 2e-4 of the gradient's max,
tests/test_train_gpu.py), and ALL images bit-equal to the same entry called on the two n = 32 halves.

Reductions (statistics partials, weight gradients): the oracle is fp64, computed on the device with plain torch ops
(nine shifted slices, one matmul each) in chunks of images, independent of the library.  No tolerance is fixed beforehand:
the entry is measured on each n = 32 half - an uncut launch - against the oracle of that half, and the full result may be
twice the larger of the two relative errors off (the row count doubles; fp32 partial sums grow at most linearly).  Inputs have
a non-zero mean so that the sums of the halves add up coherently and the full result's magnitude is about twice a half's.

One Trainer.step at 64 x 512^2 in 'f32' and in 'bf16' (whose Cin = 3 stem stays on the fp32 route): finite loss, a second run
bit-equal, the workspace exactly y3_net_train_workspace_bytes.  Before the launchers could cut, all of these raised ValueError
("tensor exceeds 2^29 elements").  Each test holds under 7 GB of device memory, the steps their workspace."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import COCO_ANCHORS, blob_images

pytestmark = pytest.mark.gpu

N, S = 64, 512
HALF = N // 2
SHOWN = (0, HALF - 1, HALF, N - 1)


def _ctx():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context()


def _rand(shape, seed, mean=0.0, std=1.0):
    from yolov3_tensorflow_amd import framework as fw
    g = torch.Generator(device=fw.default_device())
    g.manual_seed(seed)
    t = torch.randn(shape, generator=g, device=fw.default_device())
    return t.mul_(std).add_(mean)


def _weights(k, cin, cout, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)


def _pack(wt):
    fw, _lib, L, ctx = _ctx()
    k, _, cin, cout = wt.shape
    w = torch.from_numpy(wt).to(fw.default_device())
    if cin == 3:
        return w
    wp = torch.empty(k * k * cout * cin, device=w.device)
    _lib.check(L.y3_pack_conv_weights(ctx, fw.ptr(w), k, cin, cout, fw.ptr(wp)))
    return wp


def _two_ranges_of_32(L, d, dz_stride=0):
    begin, count = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    assert L.y3_conv_image_ranges(ctypes.byref(d), dz_stride, 1 << 29, 4, begin, count) == 2
    assert list(count[:2]) == [HALF, HALF] and list(begin[:2]) == [0, HALF]


def _conv64_cpu(x, wt, stride):
    """fp64 CPU conv of a few images, NHWC in and out (stride 2: explicit pad 1, utils/layer_utils.py:10-21)"""
    xd = x.double().cpu().permute(0, 3, 1, 2)
    wd = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    y = F.conv2d(F.pad(xd, (1, 1, 1, 1)), wd, stride=stride)
    return y.permute(0, 2, 3, 1).numpy()


def _taps64(x, stride):
    """the nine shifted (and strided) views of the zero-padded fp64 image chunk x [c, h, w, ci]: tap (ky, kx) -> [c, ho, wo, ci]"""
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    h, w = x.shape[1], x.shape[2]
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, xp[:, ky:ky + h:stride, kx:kx + w:stride, :]


def _conv64_dev(x, wt, stride, chunk=4):
    """fp64 conv on the device, plain ops: per image chunk, nine slices times their [ci, co] kernel planes"""
    w64 = torch.from_numpy(wt).double().to(x.device)
    for i in range(0, x.shape[0], chunk):
        acc = None
        for ky, kx, v in _taps64(x[i:i + chunk], stride):
            t = v.reshape(-1, v.shape[3]) @ w64[ky, kx]
            acc = t if acc is None else acc + t
        yield i, acc          # [chunk * ho * wo, co]


def _wgrad64_dev(x, dz, stride, lo, hi, chunk=4):
    """fp64 weight gradient over images [lo, hi) on the device, plain ops: dw[ky, kx] = sum of slice^T @ dz"""
    cin, cout = x.shape[3], dz.shape[3]
    dw = torch.zeros((3, 3, cin, cout), dtype=torch.float64, device=x.device)
    for i in range(lo, hi, chunk):
        z64 = dz[i:i + chunk].double().reshape(-1, cout)
        for ky, kx, v in _taps64(x[i:i + chunk], stride):
            dw[ky, kx] += v.reshape(-1, cin).t() @ z64
    return dw


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def _check_pixels(got, want, what):
    err = np.abs(got - want)
    assert np.isfinite(got).all(), what
    assert (err <= 1e-4 * (1 + np.abs(want))).all(), '%s: max err %.3e (max |ref| %.2f)' % (what, err.max(), np.abs(want).max())


def _fwd(d, x, wp, ones, zeros, y, stats=None):
    fw, _lib, L, ctx = _ctx()
    if stats is None:
        _lib.check(L.y3_conv2d_fwd(ctx, ctypes.byref(d), fw.ptr(x), None, fw.ptr(wp), fw.ptr(ones), fw.ptr(zeros), None,
                                   fw.ptr(y), None, ctypes.c_size_t(0)))
    else:
        _lib.check(L.y3_conv2d_fwd_stats(ctx, ctypes.byref(d), fw.ptr(x), fw.ptr(wp), fw.ptr(ones), fw.ptr(zeros), fw.ptr(y),
                                         fw.ptr(stats), None, ctypes.c_size_t(0)))


def test_stem_forward():
    """y3_conv2d_fwd, 3 -> 32 at 64 x 512 x 512: the output holds exactly 2^29 elements."""
    fw, _lib, L, ctx = _ctx()
    d = _lib.ConvDesc(N, S, S, 3, 0, 32, 3, 1, 1)
    dh = _lib.ConvDesc(HALF, S, S, 3, 0, 32, 3, 1, 1)
    _two_ranges_of_32(L, d)
    wt = _weights(3, 3, 32, 1)
    x = _rand((N, S, S, 3), 11)
    wp = _pack(wt)
    ones, zeros = torch.ones(32, device=x.device), torch.zeros(32, device=x.device)
    y = torch.empty((N, S, S, 32), device=x.device)
    assert y.numel() == 1 << 29
    _fwd(d, x, wp, ones, zeros, y)
    halves = torch.empty_like(y)
    for b in (0, HALF):
        _fwd(dh, x[b:b + HALF], wp, ones, zeros, halves[b:b + HALF])
    assert torch.equal(y, halves)
    del halves
    for i in SHOWN:
        want = _conv64_cpu(x[i:i + 1], wt, 1)
        _check_pixels(y[i:i + 1].cpu().numpy(), np.where(want > 0, want, 0.1 * want), 'image %d' % i)


def test_layer1_forward_with_statistics():
    """y3_conv2d_fwd_stats, 32 -> 64 stride 2 at 64 x 512 x 512 (the input holds 2^29 elements).  Column sums of z and z^2
    (the partial rows, added in fp64) against the fp64 device oracle; relative to the largest channel's sum:
        measured (MI355X): half 0  sum z 6.8e-10, sum z^2 1.5e-09;  half 1  sum z 1.0e-09, sum z^2 1.3e-09;
        full  sum z 7.7e-10, sum z^2 8.3e-10  (allowed: twice the larger half, 2.0e-09 and 3.0e-09)."""
    fw, _lib, L, ctx = _ctx()
    cin, cout = 32, 64
    d = _lib.ConvDesc(N, S, S, cin, 0, cout, 3, 2, 0)
    dh = _lib.ConvDesc(HALF, S, S, cin, 0, cout, 3, 2, 0)
    _two_ranges_of_32(L, d)
    wt = _weights(3, cin, cout, 2)
    x = _rand((N, S, S, cin), 12, mean=0.5)
    assert x.numel() == 1 << 29
    wp = _pack(wt)
    ones, zeros = torch.ones(cout, device=x.device), torch.zeros(cout, device=x.device)
    nb, nbh = L.y3_conv_stats_blocks(ctypes.byref(d), 0), L.y3_conv_stats_blocks(ctypes.byref(dh), 0)
    assert nb == 2 * nbh == N * (S // 2) * (S // 2) // 128
    z = torch.empty((N, S // 2, S // 2, cout), device=x.device)
    part = torch.full((nb, 2, cout), float('nan'), device=x.device)
    _fwd(d, x, wp, ones, zeros, z, part)
    zh = torch.empty_like(z)
    parth = torch.full((2, nbh, 2, cout), float('nan'), device=x.device)
    for j, b in enumerate((0, HALF)):
        _fwd(dh, x[b:b + HALF], wp, ones, zeros, zh[b:b + HALF], parth[j])
    assert torch.equal(z, zh)
    assert torch.equal(part, parth.reshape(nb, 2, cout))         # the ranges' rows, one behind the other
    del zh
    for i in SHOWN:
        _check_pixels(z[i:i + 1].cpu().numpy(), _conv64_cpu(x[i:i + 1], wt, 2), 'image %d' % i)
    # the oracle's column sums per half
    sums = torch.zeros((2, 2, cout), dtype=torch.float64, device=x.device)
    for i, z64 in _conv64_dev(x, wt, 2):
        sums[i // HALF, 0] += z64.sum(0)
        sums[i // HALF, 1] += (z64 * z64).sum(0)
    e_half = [[_rel(parth[j, :, q].double().sum(0), sums[j, q]) for q in range(2)] for j in range(2)]
    e_full = [_rel(part[:, q].double().sum(0), sums[:, q].sum(0)) for q in range(2)]
    print('layer 1 statistics: rel err of sum z, sum z^2: halves %s, full %s' % (e_half, e_full))
    for q in range(2):
        assert e_full[q] <= 2 * max(e_half[0][q], e_half[1][q])


def test_layer1_data_gradient():
    """y3_conv2d_dgrad of the 32 -> 64 stride-2 layer: dx holds 2^29 elements, four parity-class launches per range."""
    fw, _lib, L, ctx = _ctx()
    cin, cout = 32, 64
    d = _lib.ConvDesc(N, S, S, cin, 0, cout, 3, 2, 0)
    dh = _lib.ConvDesc(HALF, S, S, cin, 0, cout, 3, 2, 0)
    _two_ranges_of_32(L, d, cout)
    wt = _weights(3, cin, cout, 3)
    dz = _rand((N, S // 2, S // 2, cout), 13)
    dev = dz.device
    w_d = torch.from_numpy(wt.reshape(9 * cin, cout)).to(dev)
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)

    def run(desc, dzv, dxv):
        _lib.check(L.y3_conv2d_dgrad(ctx, ctypes.byref(desc), fw.ptr(dzv), cout, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros), 0,
                                     fw.ptr(dxv), None, ctypes.c_size_t(0)))
    dx = torch.empty((N, S, S, cin), device=dev)
    assert dx.numel() == 1 << 29
    run(d, dz, dx)
    halves = torch.empty_like(dx)
    for b in (0, HALF):
        run(dh, dz[b:b + HALF], halves[b:b + HALF])
    assert torch.equal(dx, halves)
    del halves
    wd = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    for i in SHOWN:
        xz = torch.zeros((1, cin, S, S), dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(xz, (1, 1, 1, 1)), wd, stride=2).backward(dz[i:i + 1].double().cpu().permute(0, 3, 1, 2))
        want = xz.grad.permute(0, 2, 3, 1).numpy()
        got = dx[i:i + 1].cpu().numpy()
        assert np.abs(got - want).max() < 2e-4 * np.abs(want).max(), 'image %d' % i


def _wgrad_case(cin, cout, stride, seed):
    fw, _lib, L, ctx = _ctx()
    ho = S // stride
    d = _lib.ConvDesc(N, S, S, cin, 0, cout, 3, stride, 0)
    dh = _lib.ConvDesc(HALF, S, S, cin, 0, cout, 3, stride, 0)
    _two_ranges_of_32(L, d, cout)
    x = _rand((N, S, S, cin), seed, mean=0.5)
    dz = _rand((N, ho, ho, cout), seed + 1, mean=0.25)
    dev = x.device

    def run(desc, xv, dzv):
        nbytes = L.y3_conv_wgrad_scratch_bytes(ctypes.byref(desc))
        sc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dw = torch.full((3, 3, cin, cout), float('nan'), device=dev)
        _lib.check(L.y3_conv_wgrad(ctx, ctypes.byref(desc), fw.ptr(xv), fw.ptr(dzv), cout, fw.ptr(dw), fw.ptr(sc),
                                   ctypes.c_size_t(nbytes)))
        return dw
    full, again = run(d, x, dz), run(d, x, dz)
    assert torch.equal(full, again), 'not run-to-run bit-exact'
    want_h = [_wgrad64_dev(x, dz, stride, b, b + HALF) for b in (0, HALF)]
    e_half = [_rel(run(dh, x[b:b + HALF], dz[b:b + HALF]), want_h[j]) for j, b in enumerate((0, HALF))]
    e_full = _rel(full, want_h[0] + want_h[1])
    print('weight gradient %d -> %d stride %d: rel err halves %s, full %.3e' % (cin, cout, stride, e_half, e_full))
    assert e_full <= 2 * max(e_half)


def test_layer1_weight_gradient():
    """y3_conv_wgrad, 32 -> 64 stride 2: x holds 2^29 elements; the splits of both ranges added by one sum kernel.
        measured (MI355X), relative to the gradient's largest element: halves 5.5e-07 and 5.3e-07, full 4.7e-07
        (allowed: twice the larger half, 1.1e-06)."""
    _wgrad_case(32, 64, 2, 21)


def test_stem_weight_gradient():
    """y3_conv_wgrad's stem path, 3 -> 32: dz holds 2^29 elements; 2 x 1536 workgroup partials, one sum kernel.
        measured (MI355X), relative to the gradient's largest element: halves 1.9e-07 and 1.5e-07, full 2.5e-07
        (allowed: twice the larger half, 3.8e-07)."""
    _wgrad_case(3, 32, 1, 31)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_one_train_step_at_batch_64_512px(dtype, isolated_graph):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training, _lib, framework as fw
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    from oracle import yolo_ref, train_ref
    from test_train_gpu import _fresh_model
    L = _lib.lib()
    params = yolo_ref.synthetic_params(80, seed=3)
    x = blob_images(9, N, S)
    yts = train_ref.synthetic_targets(10, N, [S, S], 80, COCO_ANCHORS, max_boxes=4)
    runs = []
    for _ in range(2):
        model = _fresh_model(params, batch_norm_decay=0.99, weight_decay=5e-4)
        model.compute_dtype = dtype
        trainer = training.Trainer(model, config_optimizer('momentum', 1e-4), wgrad_stream=True)
        with y3.variable_scope('yolov3'):
            loss = [float(v) for v in trainer.step(x, yts)]
        fw.check_context()
        st = training._train_state(model)
        net = training._train_net(model, fw.context(), fw.default_device())
        assert st['ws'].numel() == L.y3_net_train_workspace_bytes(net, st['vars_all'], N, S, S) > (1 << 31)
        assert all(np.isfinite(v) for v in loss), loss
        runs.append((loss, trainer.flat.clone()))
        del trainer, model
        st['ws'] = None
    assert runs[0][0] == runs[1][0]
    assert torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][1], runs[1][1])
