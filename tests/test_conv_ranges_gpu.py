"""GPU: the fp32 conv launchers cut into image ranges at small shapes, under a limit lowered by the test hook
y3_debug_conv_range_limit (restored in a `finally` everywhere).  n = 5 images and a limit of two images plus one element:
ranges of 2, 2 and 1 images.  Every op is compared with the same entry with the hook off; reductions (statistics partials,
fused BN-backward partials, weight gradients) against fp64 from the same inputs at the tolerances of
tests/test_train_gpu.py, and run twice for bit equality.  The whole step: _step_matches_oracle of tests/test_train_gpu.py,
unchanged, under a limit of 3,000,000 elements.

Stream-K: a cut launch never takes that schedule (its ranges run without a workspace), so the case whose ranges alone would
take it checks that they do not: bit-equal to the data-parallel whole launch, and within tests/test_conv_gpu.py's tolerance
of fp64 - which is also how far the cut result may lie from the stream-K whole launch."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_gpu import ref_conv, make_case, check

pytestmark = pytest.mark.gpu

N = 5
SK_WS = 512 * 128 * 128 * 4 + 512 * 4


def _ctx():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context()


@contextlib.contextmanager
def lowered(elements):
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    L.y3_debug_conv_range_limit(elements)
    try:
        yield
    finally:
        L.y3_debug_conv_range_limit(0)


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))


def two_image_limit(d, dz_stride=0):
    co = dz_stride or d.cout
    return 2 * max(d.h * d.w * d.cin, (d.h // d.stride) * (d.w // d.stride) * co) + 1


def assert_cut(L, d, dz_stride, limit, want=(2, 2, 1)):
    begin, count = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    nr = L.y3_conv_image_ranges(ctypes.byref(d), dz_stride, limit, 8, begin, count)
    assert tuple(count[:nr]) == want


def _gpu(a):
    from yolov3_tensorflow_amd import framework as fw
    return torch.from_numpy(np.ascontiguousarray(a)).to(fw.default_device())


def _pack(wt, planes=0):
    fw, _lib, L, ctx = _ctx()
    k, _, cin, cout = wt.shape
    w = _gpu(wt)
    if cin == 3:
        return w
    if planes:
        wp = torch.empty(planes * k * k * cout * cin, device=w.device, dtype=torch.bfloat16)
        _lib.check(L.y3_pack_conv_weights_split(ctx, fw.ptr(w), k, cin, cout, planes, fw.ptr(wp)))
    else:
        wp = torch.empty(k * k * cout * cin, device=w.device)
        _lib.check(L.y3_pack_conv_weights(ctx, fw.ptr(w), k, cin, cout, fw.ptr(wp)))
    return wp


def _fwd(d, xg, wp, sg, hg, planes=0, resid=None, stats=None, workspace=True):
    fw, _lib, L, ctx = _ctx()
    y = torch.full((d.n, d.h // d.stride, d.w // d.stride, d.cout), float('nan'), device=xg.device)
    ws = torch.empty(SK_WS, dtype=torch.uint8, device=xg.device) if workspace else None
    wsb = ctypes.c_size_t(SK_WS if workspace else 0)
    if planes:
        _lib.check(L.y3_conv2d_fwd_split(ctx, ctypes.byref(d), planes, fw.ptr(xg), None, fw.ptr(wp), fw.ptr(sg), fw.ptr(hg),
                                         fw.ptr(resid), fw.ptr(y), fw.ptr(ws), wsb))
    elif stats is not None:
        _lib.check(L.y3_conv2d_fwd_stats(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(wp), fw.ptr(sg), fw.ptr(hg), fw.ptr(y),
                                         fw.ptr(stats), fw.ptr(ws), wsb))
    else:
        _lib.check(L.y3_conv2d_fwd(ctx, ctypes.byref(d), fw.ptr(xg), None, fw.ptr(wp), fw.ptr(sg), fw.ptr(hg), fw.ptr(resid),
                                   fw.ptr(y), fw.ptr(ws), wsb))
    return y


# (name, h, w, k, stride, cin, cout, planes, residual)
FWD = [
    ('3x3 s1', 32, 32, 3, 1, 32, 64, 0, True),
    ('3x3 s2', 48, 32, 3, 2, 32, 64, 0, False),
    ('3x3 s2 odd rows', 26, 30, 3, 2, 64, 128, 0, False),      # 195 rows per image: ranges end inside a tile of the whole
    ('1x1 128-row tiles', 48, 32, 1, 1, 64, 32, 0, False),
    ('1x1 64x64 tiles', 32, 32, 1, 1, 256, 128, 0, True),
    ('1x1 odd cout', 13, 13, 1, 1, 256, 255, 0, False),
    ('stem', 48, 32, 3, 1, 3, 32, 0, False),
    ('stem odd', 33, 37, 3, 1, 3, 32, 0, False),                # 1221 pixels per image: ranges end inside a 256-pixel block
    ('split x6', 32, 32, 3, 1, 32, 64, 3, True),
    ('split x3 s2', 48, 32, 3, 2, 32, 64, 2, False),
    ('split x6 1x1', 48, 32, 1, 1, 64, 32, 3, False),
]


@pytest.mark.parametrize('case', range(len(FWD)), ids=[c[0] for c in FWD])
def test_forward_cut_equals_the_single_launch(case):
    fw, _lib, L, ctx = _ctx()
    name, h, w, k, stride, cin, cout, planes, resid = FWD[case]
    rng = np.random.RandomState(700 + case)
    x, wt, scale, shift = make_case(rng, N, h, w, k, cin, cout)
    r = rng.standard_normal((N, h // stride, w // stride, cout)).astype(np.float32) if resid else None
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, k, stride, 1)
    limit = two_image_limit(d)
    xg, sg, hg, rg, wp = _gpu(x), _gpu(scale), _gpu(shift), None if r is None else _gpu(r), _pack(wt, planes)
    assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) != 1
    whole = _fwd(d, xg, wp, sg, hg, planes, rg)
    with lowered(limit):
        assert_cut(L, d, 0, limit)
        cut = _fwd(d, xg, wp, sg, hg, planes, rg)
        again = _fwd(d, xg, wp, sg, hg, planes, rg)
    assert torch.equal(cut, whole), name
    assert torch.equal(cut, again)
    check(cut.cpu().numpy(), ref_conv(x, wt, scale, shift, k, stride, True, r), name, planes)


@pytest.mark.parametrize('planes', [0, 3])
def test_a_range_that_alone_would_take_stream_k_runs_data_parallel(planes):
    """5 x 32 x 32, 64 -> 256: the whole launch (80 tiles) and a range of two images alone (32 tiles) both take stream-K when
    given a workspace.  Cut, no range does: the result is the data-parallel whole launch bit for bit, y3_conv_schedule says 0,
    and it stays within the forward tolerance of fp64 (as the stream-K whole launch does)."""
    fw, _lib, L, ctx = _ctx()
    h = w = 32
    cin, cout = 64, 256
    rng = np.random.RandomState(77)
    x, wt, scale, shift = make_case(rng, N, h, w, 3, cin, cout)
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, 3, 1, 1)
    two = _lib.ConvDesc(2, h, w, cin, 0, cout, 3, 1, 1)
    assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) == 1 and L.y3_conv_schedule(ctypes.byref(two), 0, 1) == 1
    xg, sg, hg, wp = _gpu(x), _gpu(scale), _gpu(shift), _pack(wt, planes)
    whole_sk = _fwd(d, xg, wp, sg, hg, planes)
    whole_dp = _fwd(d, xg, wp, sg, hg, planes, workspace=False)
    limit = two_image_limit(d)
    with lowered(limit):
        assert_cut(L, d, 0, limit)
        assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) == 0
        assert L.y3_conv_workspace_bytes(ctypes.byref(d)) == 0
        cut = _fwd(d, xg, wp, sg, hg, planes)
    assert torch.equal(cut, whole_dp)
    want = ref_conv(x, wt, scale, shift, 3, 1, True)
    check(cut.cpu().numpy(), want, 'cut', planes)
    check(whole_sk.cpu().numpy(), want, 'stream-K whole', planes)
    _lib.check(L.y3_ctx_check(ctx))


# the FORWARD layer (name, h, w, k, stride, cin, cout, dz_stride)
DGRAD = [
    ('3x3 s1', 32, 32, 3, 1, 32, 64, 64),
    ('3x3 s2 parity classes', 48, 32, 3, 2, 32, 64, 64),
    ('3x3 s2 odd rows', 26, 30, 3, 2, 64, 128, 128),
    ('1x1', 48, 32, 1, 1, 64, 32, 32),
    ('1x1 detection', 13, 13, 1, 1, 256, 255, 256),
]


def _dgrad64(dz, wt, x_shape, k, stride):
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    xp = x.permute(0, 3, 1, 2)
    wd = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    z = F.conv2d(F.pad(xp, (1, 1, 1, 1)), wd, stride=stride) if stride > 1 else F.conv2d(xp, wd, padding=k // 2)
    z.backward(torch.from_numpy(dz).double().permute(0, 3, 1, 2))
    return x.grad.numpy()


@pytest.mark.parametrize('case', range(len(DGRAD)), ids=[c[0] for c in DGRAD])
def test_data_gradient_cut_equals_the_single_launch(case):
    fw, _lib, L, ctx = _ctx()
    name, h, w, k, stride, cin, cout, dzs = DGRAD[case]
    rng = np.random.RandomState(800 + case)
    ho, wo = h // stride, w // stride
    dz = rng.standard_normal((N, ho, wo, cout)).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((N, h, w, cin)).astype(np.float32)
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, k, stride, 0)
    limit = two_image_limit(d, dzs)
    dzp = np.zeros((N, ho, wo, dzs), np.float32)
    dzp[..., :cout] = dz
    dzg, pg = _gpu(dzp), _gpu(prior)
    dev = dzg.device
    w_d = torch.zeros((k * k * cin, dzs), device=dev)
    w_d[:, :cout] = _gpu(wt.reshape(k * k * cin, cout))
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    ws = torch.empty(SK_WS, dtype=torch.uint8, device=dev)
    want = _dgrad64(dz, wt, (N, h, w, cin), k, stride)

    def run(entry, wk, acc, *lead):
        dx = pg.clone() if acc else torch.full((N, h, w, cin), float('nan'), device=dev)
        _lib.check(entry(ctx, ctypes.byref(d), *lead, fw.ptr(dzg), dzs, fw.ptr(wk), fw.ptr(ones), fw.ptr(zeros), acc, fw.ptr(dx),
                         fw.ptr(ws), ctypes.c_size_t(SK_WS)))
        return dx
    entries = [(L.y3_conv2d_dgrad, w_d, (), 2e-4)]
    if stride == 1:
        wsd = torch.empty(3 * k * k * cin * dzs, dtype=torch.bfloat16, device=dev)
        _lib.check(L.y3_pack_conv_weights_split_dgrad(ctx, fw.ptr(w_d), k, cin, dzs, 3, fw.ptr(wsd)))
        entries.append((L.y3_conv2d_dgrad_split, wsd, (3,), 2e-4))
    for entry, wk, lead, tol in entries:
        for acc in (0, 1):
            whole = run(entry, wk, acc, *lead)
            with lowered(limit):
                assert_cut(L, d, dzs, limit)
                cut = run(entry, wk, acc, *lead)
            assert torch.equal(cut, whole), '%s accumulate=%d' % (name, acc)
            assert rel_err(cut.cpu().numpy(), want + (prior if acc else 0.0)) < tol


# ---- reductions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,k,stride,cin,cout', [
    (32, 32, 3, 1, 32, 64), (48, 32, 3, 2, 32, 64), (26, 30, 3, 2, 64, 128), (48, 32, 1, 1, 64, 32), (33, 31, 1, 1, 256, 128)])
def test_statistics_partials_of_a_cut_launch(h, w, k, stride, cin, cout):
    """y3_conv2d_fwd_stats cut into ranges: z bit-equal to the single launch; the partial rows - every range's behind the
    previous range's, y3_conv_stats_blocks of them - finalised by ONE y3_bn_train_stats_partials against fp64 statistics of
    the same z at test_conv_epilogue_statistics_equal_the_separate_pass's tolerances; two runs bit-equal."""
    fw, _lib, L, ctx = _ctx()
    rng = np.random.RandomState(900 + h + cin)
    x, wt, _, _ = make_case(rng, N, h, w, k, cin, cout)
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, k, stride, 0)
    limit = two_image_limit(d)
    xg, wp = _gpu(x), _pack(wt)
    dev = xg.device
    ones, zeros = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    gamma, beta = _gpu(rng.uniform(0.5, 1.5, cout).astype(np.float32)), _gpu(rng.normal(0, 0.3, cout).astype(np.float32))
    rows_img = (h // stride) * (w // stride)
    bm = 64 if (k == 1 and cout > 64) else 128
    nb_whole = L.y3_conv_stats_blocks(ctypes.byref(d), 0)
    assert nb_whole == -(-N * rows_img // bm)
    z_whole = _fwd(d, xg, wp, ones, zeros, stats=torch.empty((nb_whole, 2, cout), device=dev))
    outs = []
    with lowered(limit):
        assert_cut(L, d, 0, limit)
        nblk = L.y3_conv_stats_blocks(ctypes.byref(d), 0)
        assert nblk == 2 * -(-2 * rows_img // bm) + -(-rows_img // bm)
        for _ in range(2):
            part = torch.full((nblk + 1, 2, cout), float('nan'), device=dev)
            z = _fwd(d, xg, wp, ones, zeros, stats=part)
            assert torch.isnan(part[nblk]).all() and torch.isfinite(part[:nblk]).all()      # exactly the rows the query counts
            st = torch.empty((4, cout), device=dev)
            _lib.check(L.y3_bn_train_stats_partials(ctx, fw.ptr(part), nblk, N * rows_img, cout, fw.ptr(gamma), fw.ptr(beta),
                                                    ctypes.c_float(1e-5), ctypes.c_float(0.9), fw.ptr(st[0]), fw.ptr(st[1]),
                                                    fw.ptr(st[2]), fw.ptr(st[3]), None, None))
            outs.append((z, part[:nblk].clone(), st))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b), 'not run-to-run bit-exact'
    z, part, st = outs[0]
    assert torch.equal(z, z_whole)
    zz = z.double().reshape(-1, cout)
    mean64, var64 = zz.mean(0), zz.var(0, unbiased=False)
    assert float((st[0].double() - mean64).abs().max()) <= 1e-5 * float(zz.abs().max())
    np.testing.assert_allclose(st[1].cpu().numpy(), (1.0 / torch.sqrt(var64 + 1e-5)).cpu().numpy(), rtol=2e-5)
    # every range's rows hold that range's pixels: the first range's blocks sum to the sums of images 0 and 1
    nb0 = -(-2 * rows_img // bm)
    s0 = part[:nb0, 0].double().sum(0)
    want0 = zz[:2 * rows_img].sum(0)
    assert float((s0 - want0).abs().max()) <= 1e-5 * float(zz[:2 * rows_img].abs().sum(0).max())


@pytest.mark.parametrize('h,w,cin,cout,dzs', [(48, 32, 64, 32, 32), (33, 31, 128, 64, 64), (13, 13, 256, 255, 256)])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_fused_bn_backward_partials_of_a_cut_launch(h, w, cin, cout, dzs, accumulate):
    """y3_conv2d_dgrad_bn cut into ranges: dx bit-equal to the single launch, the partial rows (y3_conv_dgrad_bn_blocks of
    them, range-major) summed in fp64 against fp64 sums of g' and g' * zhat over the stored dx (2e-4 of the larger sum's
    magnitude, the data gradient's tolerance), y3_bn_train_bwd_partials on them against y3_bn_train_bwd; two runs bit-equal."""
    fw, _lib, L, ctx = _ctx()
    m_img = h * w
    m = N * m_img
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, 1, 1, 0)
    limit = two_image_limit(d, dzs)
    rng = np.random.RandomState(950 + cin)
    z = (rng.standard_normal((m, cin)) * 2 + rng.standard_normal(cin)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.normal(0, 0.3, cin).astype(np.float32)
    dz = np.zeros((m, dzs), np.float32)
    dz[:, :cout] = rng.standard_normal((m, cout))
    wt = (rng.standard_normal((cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((m, cin)).astype(np.float32)
    zg, gg, bg, pg, dzg = _gpu(z), _gpu(gamma), _gpu(beta), _gpu(prior), _gpu(dz)
    dev = zg.device
    vec = torch.empty((4, cin), device=dev)
    sc = torch.empty(L.y3_bn_bwd_scratch_bytes(cin), dtype=torch.uint8, device=dev)
    _lib.check(L.y3_bn_train_stats(ctx, fw.ptr(zg), m, cin, fw.ptr(gg), fw.ptr(bg), ctypes.c_float(1e-5), ctypes.c_float(0.9),
                                   fw.ptr(vec[0]), fw.ptr(vec[1]), fw.ptr(vec[2]), fw.ptr(vec[3]), None, None, fw.ptr(sc)))
    mean, istd, scale, shift = vec.cpu().numpy()
    w_d = torch.zeros((cin, dzs), device=dev)
    w_d[:, :cout] = _gpu(wt)
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    bm = 64 if cin > 64 else 128

    def run(nblk):
        dx = pg.clone() if accumulate else torch.full((m, cin), float('nan'), device=dev)
        part = torch.full((nblk + 1, 2, cin), float('nan'), device=dev)
        _lib.check(L.y3_conv2d_dgrad_bn(ctx, ctypes.byref(d), fw.ptr(dzg), dzs, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros),
                                        accumulate, fw.ptr(dx), fw.ptr(zg), fw.ptr(vec), fw.ptr(part)))
        assert torch.isnan(part[nblk]).all() and torch.isfinite(part[:nblk]).all()
        return dx, part[:nblk].contiguous()
    dx_whole, _ = run(L.y3_conv_dgrad_bn_blocks(ctypes.byref(d)))
    with lowered(limit):
        assert_cut(L, d, dzs, limit)
        nblk = L.y3_conv_dgrad_bn_blocks(ctypes.byref(d))
        assert nblk == 2 * -(-2 * m_img // bm) + -(-m_img // bm)
        (dx, part), (dx2, part2) = run(nblk), run(nblk)
        res = []
        for fused in (True, False):
            dgam, dbet = torch.empty(cin, device=dev), torch.empty(cin, device=dev)
            dzo = torch.empty((m, cin), device=dev)
            if fused:
                _lib.check(L.y3_bn_train_bwd_partials(ctx, fw.ptr(zg), fw.ptr(dx), fw.ptr(gg), fw.ptr(vec[2]), fw.ptr(vec[3]),
                                                      fw.ptr(vec[0]), fw.ptr(vec[1]), m, cin, fw.ptr(part), nblk, fw.ptr(dgam),
                                                      fw.ptr(dbet), fw.ptr(dzo), fw.ptr(sc)))
            else:
                _lib.check(L.y3_bn_train_bwd(ctx, fw.ptr(zg), fw.ptr(dx), fw.ptr(gg), fw.ptr(vec[2]), fw.ptr(vec[3]), fw.ptr(vec[0]),
                                             fw.ptr(vec[1]), m, cin, fw.ptr(dgam), fw.ptr(dbet), fw.ptr(dzo), fw.ptr(sc)))
            res.append([t.cpu().numpy().astype(np.float64) for t in (dgam, dbet, dzo)])
    assert torch.equal(dx, dx2) and torch.equal(part, part2), 'not run-to-run bit-exact'
    assert torch.equal(dx, dx_whole)
    mask = (z * scale + shift) > 0
    g = dx.cpu().numpy().astype(np.float64) * np.where(mask, 1.0, np.float64(np.float32(0.1)))
    zhat = (z.astype(np.float64) - mean.astype(np.float64)) * istd.astype(np.float64)
    got = part.cpu().numpy().astype(np.float64).sum(0)
    for j, want in enumerate((g.sum(0), (g * zhat).sum(0))):
        assert rel_err(got[j], want) < 2e-4
    for a, b in zip(*res):
        assert rel_err(a, b) < 2e-4


@pytest.mark.parametrize('h,w,k,stride,cin,cout,dzs', [
    (32, 32, 3, 1, 32, 64, 64), (48, 32, 3, 2, 32, 64, 64), (26, 30, 3, 2, 64, 128, 128), (48, 32, 1, 1, 64, 32, 32),
    (13, 13, 1, 1, 256, 255, 256),
    (48, 32, 3, 1, 3, 32, 32), (33, 130, 3, 1, 3, 32, 32),      # the stem path: whole pieces, and a last piece of 2 pixels
])
def test_weight_gradient_of_a_cut_launch(h, w, k, stride, cin, cout, dzs):
    """y3_conv_wgrad cut into ranges: every range's split partials in its own region of the scratch, one sum kernel over all
    of them.  Against fp64 autograd at test_conv_wgrad_and_dgrad_match_autograd's 2e-4; two runs bit-equal; a scratch one
    byte short of y3_conv_wgrad_scratch_bytes is refused."""
    fw, _lib, L, ctx = _ctx()
    rng = np.random.RandomState(1000 + h + cin)
    x = torch.tensor(rng.standard_normal((N, h, w, cin)), dtype=torch.float64)
    wt = torch.zeros((k, k, cin, cout), dtype=torch.float64, requires_grad=True)
    xp = x.permute(0, 3, 1, 2)
    z = F.conv2d(F.pad(xp, (1, 1, 1, 1)), wt.permute(3, 2, 0, 1), stride=stride) if stride > 1 else \
        F.conv2d(xp, wt.permute(3, 2, 0, 1), padding=k // 2)
    ho, wo = z.shape[2], z.shape[3]
    dz = rng.standard_normal((N, ho, wo, cout))
    z.backward(torch.tensor(dz).permute(0, 3, 1, 2))
    want = wt.grad.numpy()
    dzp = np.zeros((N, ho, wo, dzs), np.float32)
    dzp[..., :cout] = dz
    d = _lib.ConvDesc(N, h, w, cin, 0, cout, k, stride, 0)
    limit = two_image_limit(d, dzs)
    xg, dzg = _gpu(x.numpy().astype(np.float32)), _gpu(dzp)
    dev = xg.device

    def run(short=0):
        nbytes = L.y3_conv_wgrad_scratch_bytes(ctypes.byref(d))
        sc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dw = torch.full((k, k, cin, cout), float('nan'), device=dev)
        rc = L.y3_conv_wgrad(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(dzg), dzs, fw.ptr(dw), fw.ptr(sc),
                             ctypes.c_size_t(nbytes - short))
        return rc, dw, nbytes
    rc, whole, whole_bytes = run()
    _lib.check(rc)
    with lowered(limit):
        assert_cut(L, d, dzs, limit)
        (rc1, cut, cut_bytes), (rc2, again, _) = run(), run()
        _lib.check(rc1)
        _lib.check(rc2)
        assert run(short=1)[0] == _lib.Y3_EINVAL
    assert cut_bytes >= whole_bytes
    assert torch.equal(cut, again), 'not run-to-run bit-exact'
    assert rel_err(cut.cpu().numpy(), want) < 2e-4
    assert rel_err(whole.cpu().numpy(), want) < 2e-4


# ---- the whole step -------------------------------------------------------------------------------------------------------
STEP_LIMIT = 3000000      # 256 px, bs = 4: cuts layers 0-3 (tensors of 8.4, 4.2 and 2.1 M elements), a fused dgrad-BN layer among them


@pytest.mark.parametrize('optimizer,update_scopes,dtype,wgrad_stream', [
    ('sgd', None, 'f32', 'auto'), ('sgd', None, 'f32_bf16x6', 'auto'), ('momentum', None, 'f32_wino', 'auto'),
    ('sgd', None, 'f32', True)])      # ... and with every weight gradient, all its ranges, on the second stream
def test_one_train_step_with_cut_layers_matches_oracle(optimizer, update_scopes, dtype, wgrad_stream, isolated_graph):
    from test_train_gpu import _step_matches_oracle
    fw, _lib, L, ctx = _ctx()
    for cin, cout, k, stride, size in ((3, 32, 3, 1, 256), (32, 64, 3, 2, 256), (64, 32, 1, 1, 128)):
        d = _lib.ConvDesc(4, size, size, cin, 0, cout, k, stride, 1)
        begin, count = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
        assert L.y3_conv_image_ranges(ctypes.byref(d), 0, STEP_LIMIT, 8, begin, count) > 1
    with lowered(STEP_LIMIT):
        _step_matches_oracle(optimizer, update_scopes, dtype, wgrad_stream, 'cut at %d' % STEP_LIMIT)
