"""The schedules of the fp32 conv family that the cheap per-kernel shapes never reach, each against an fp64 torch-CPU conv or
autograd of the same fp32 inputs (x, dz ~ N(0,1); weights ~ N(0, 0.1) or He-scaled, as the neighbouring tests draw them):

  1. y3_conv_wgrad with several K-steps per split (the double-buffered K loop's second trip, the ragged last split, several
     hundred splits through the sum kernel), on every tile width, both strides, 1x1 convs and the detection widths;
  2. y3_conv2d_dgrad / y3_conv2d_dgrad_split on stream-K, stride 1 and the stride-2 parity classes, accumulate 0 and 1;
  3. the resident 64x64 walk of the 1x1 forward convs, at and around its thresholds, with the statistics epilogue;
  4. the BN backward reduction fused into the 1x1 data gradient's epilogue (y3_conv2d_dgrad_bn, y3_bn_train_bwd_partials).

Every case asserts the schedule it is named for (y3_conv_schedule, the weight gradient's split count) BEFORE it launches:
a case that fell back to one workgroup per tile fails.  tests/conv_schedule_cases.py holds the shapes,
tests/test_conv_schedules_cpu.py pins their schedules without a device.  Outputs (and the scratch the kernels publish
partial results through) start NaN-filled where the call overwrites them.

Gates.  Weight gradient: 2e-4 of the tensor's max (test_train_gpu.py).  Data gradient, exact kernel and the three-plane
split: elementwise |d| <= 1e-4 * (1 + |ref|), the forward kernel's gate in test_conv_gpu.py (stated there for K <= 4608; K
here is <= 2304); the two-plane split: 5e-3 of max (test_train_gpu.py).  Forward: test_conv_gpu.check.  The fused
reduction's partial sums: GATE_B below.

Guards (section 5 of each test; no broken kernel runs): references with ONE thing wrong are built on the CPU from the fp64
reference and must lie more than GUARD gates away from what the GPU produced, on the case that exists to catch that fault.
Each distance is printed (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_schedule_cases as C
from test_conv_gpu import check as fwd_check, make_case, ref_conv

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # unit roundoff of fp32
GUARD = 10.0                   # a wrong variant must be more than GUARD gates away from the GPU's result
WS_BYTES = 512 * 2 * 128 * 128 * 4     # >= the stream-K workspace (512 accumulator slots + 512 flag words)
# The fused reduction's partial sums against fp64 sums over the same block of the dx the GPU stored.  Ceiling: the bound of a
# sum of n fp32 terms taken in ANY order, each term carrying up to three roundings of its own:
#     |err| <= (rows_in_block + 3) * 2^-24 * sum |terms|     per block and column.
# Measured on an MI355X, the worst ratio to that bound over every block, column and both sums: 0.131 / 0.138 / 0.149 /
# 0.049 / 0.116 for the five cases with accumulate = 0 and 0.099 / 0.117 / 0.098 / 0.040 / 0.117 with accumulate = 1
# (MEASURED_B is the largest).  The gate is three times that, and never above the bound.
MEASURED_B = 0.149
GATE_B = min(3 * MEASURED_B, 1.0)

# which wrong variant each case exists to catch
GUARDS_WGRAD = {0: ('kstep_dropped_from_one_tile', 'ragged_last_kstep_dropped'),      # 1x1, 32-wide tile, M % 32 = 4
                3: ('kstep_dropped_from_one_tile', 'ragged_last_kstep_dropped')}      # 3x3, 128-wide tile, M % 32 = 11
GUARDS_DGRAD_S1 = ('kstep_dropped_from_one_tile', 'prior_added_twice')
GUARDS_DGRAD_S2 = ('parity_class_with_anothers_taps', 'kstep_dropped_from_one_tile', 'prior_added_twice')
GUARDS_BN = ('prior_added_twice', 'prior_left_out_of_g', 'partial_written_to_next_block', 'partial_written_to_previous_block',
             'mask_from_fp64_u')


def _ctx():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context()


def _gpu(a):
    from yolov3_tensorflow_amd import framework as fw
    return torch.from_numpy(np.ascontiguousarray(a)).to(fw.default_device())


def _nan_bytes(nbytes):
    """Scratch whose every float reads as NaN (0xffffffff): a partial result that is read before it was written shows."""
    from yolov3_tensorflow_amd import framework as fw
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=fw.default_device())


def _report(what, name, dist):
    print('guard %-28s %-36s %10.1f gates' % (what, name, dist))
    assert dist > GUARD, '%s: the variant "%s" is only %.2f gates from the GPU result' % (what, name, dist)


# ---- fp64 references -----------------------------------------------------------------------------------------------------
def _conv64(x, w, k, stride):
    """x NHWC, w HWIO (fp64 tensors) -> NCHW; explicit pad for stride 2 (utils/layer_utils.py:10-21), SAME for stride 1."""
    xp = x.permute(0, 3, 1, 2)
    if stride > 1:
        return F.conv2d(F.pad(xp, (1, 1, 1, 1)), w.permute(3, 2, 0, 1), stride=stride)
    return F.conv2d(xp, w.permute(3, 2, 0, 1), padding=k // 2)


def wgrad64(x, dz, k, stride):
    """dw [k,k,cin,cout] in fp64 from fp32 x [n,h,w,cin] and dz [n,ho,wo,cout] (linear in dz: the guards mask dz)."""
    cin, cout = x.shape[3], dz.shape[3]
    if k == 1:
        return (x.reshape(-1, cin).astype(np.float64).T @ dz.reshape(-1, cout).astype(np.float64)).reshape(1, 1, cin, cout)
    w = torch.zeros((k, k, cin, cout), dtype=torch.float64, requires_grad=True)
    z = _conv64(torch.from_numpy(x).double(), w, k, stride)
    return torch.autograd.grad(z, w, torch.from_numpy(dz).double().permute(0, 3, 1, 2))[0].numpy()


def dgrad64(dz, w, shape, k, stride):
    """dx [n,h,w,cin] in fp64 from fp32 dz [n,ho,wo,cout] and w [k,k,cin,cout] (linear in w: the guards mask w)."""
    if k == 1:
        return (dz.reshape(-1, dz.shape[3]).astype(np.float64) @ w.reshape(w.shape[2], -1).astype(np.float64).T).reshape(shape)
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    z = _conv64(x, torch.from_numpy(w).double(), k, stride)
    return torch.autograd.grad(z, x, torch.from_numpy(dz).double().permute(0, 3, 1, 2))[0].numpy()


def _pad_lanes(rng, dz, stride_c):
    """dz with its rows widened to stride_c: the lanes behind cout hold finite junk (the loss leaves them as they were)."""
    out = rng.standard_normal(dz.shape[:3] + (stride_c,)).astype(np.float32)
    out[..., :dz.shape[3]] = dz
    return out


def _elementwise_gate(want):
    return 1e-4 * (1 + np.abs(want))


def _check_elementwise(got, want, what):
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    assert (err <= _elementwise_gate(want)).all(), '%s: max err %.3e (max |ref| %.2f)' % (what, err.max(), np.abs(want).max())


def _check_of_max(got, want, tol, what):
    assert np.isfinite(got).all(), what
    e = np.abs(got - want).max() / np.abs(want).max()
    assert e < tol, '%s: %.3e of max' % (what, e)


# ==== 1. weight gradient with several K-steps per split ===================================================================
@pytest.mark.parametrize('case', range(len(C.WGRAD)))
def test_weight_gradient_with_several_k_steps_per_split(case):
    fw, _lib, L, ctx = _ctx()
    n, h, w, k, s, cin, cout, dzs, ragged = C.WGRAD[case]
    ho, wo = h // s, w // s
    m = n * ho * wo
    nsplit, chunk, last, mrem = C.wgrad_split(L, n, h, w, k, s, cin, cout)
    assert -(-m // 32) / nsplit > 1 and chunk > 1, 'one K-step per split: the K loop takes no second trip'
    if ragged is not None:
        assert 0 < last < chunk, 'the last split is not ragged'
    rng = np.random.RandomState(100 + case)
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    dz = rng.standard_normal((n, ho, wo, cout)).astype(np.float32)
    want = wgrad64(x, dz, k, s)
    d = C.desc(n, h, w, cin, 0, cout, k, s)
    xg, dzg = _gpu(x), _gpu(_pad_lanes(rng, dz, dzs))
    nbytes = L.y3_conv_wgrad_scratch_bytes(ctypes.byref(d))
    outs = []
    for _ in range(2):
        dw = torch.full((k, k, cin, cout), float('nan'), device=xg.device)
        sc = _nan_bytes(nbytes)
        _lib.check(L.y3_conv_wgrad(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(dzg), dzs, fw.ptr(dw), fw.ptr(sc),
                                   ctypes.c_size_t(nbytes)))
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), 'not run-to-run bit-exact'
    got = outs[0].cpu().numpy()
    _check_of_max(got, want, 2e-4, 'wgrad %d splits x %d K-steps' % (nsplit, chunk))
    if L.y3_conv_wgrad_wino_eligible(ctypes.byref(d)):
        dww = torch.full((k, k, cin, cout), float('nan'), device=xg.device)
        scw = _nan_bytes(L.y3_conv_wgrad_wino_scratch_bytes(ctypes.byref(d)))
        _lib.check(L.y3_conv_wgrad_wino(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(dzg), dzs, fw.ptr(dww), fw.ptr(scw),
                                        ctypes.c_size_t(scw.numel())))
        _check_of_max(dww.cpu().numpy(), want, 2e-4, 'Winograd wgrad')
        _check_of_max(dww.cpu().numpy(), got, 2e-4, 'Winograd wgrad against the direct kernel')
    else:
        assert not (k == 3 and s == 1 and cin % 64 == 0 and cout % 64 == 0)

    # ---- 5. guards ----
    if case not in GUARDS_WGRAD:
        return
    gate = 2e-4 * np.abs(want).max()
    bn = 128 if cout > 64 else 64 if cout > 32 else 32            # the kernel's tile: 128 rows of J = k*k*cin x bn columns
    variants = {}
    mask = np.zeros((m, 1), np.float32)
    t0 = chunk + 1                                                  # the second K-step of the second split
    mask[32 * t0:32 * t0 + 32] = 1
    delta = wgrad64(x, (dz.reshape(m, cout) * mask).reshape(dz.shape), k, s).reshape(-1, cout)
    v = want.reshape(-1, cout).copy()
    v[:128, :bn] -= delta[:128, :bn]
    variants['kstep_dropped_from_one_tile'] = v.reshape(want.shape)
    assert mrem > 0
    mask[:] = 0
    mask[m - mrem:] = 1
    variants['ragged_last_kstep_dropped'] = want - wgrad64(x, (dz.reshape(m, cout) * mask).reshape(dz.shape), k, s)
    assert sorted(variants) == sorted(GUARDS_WGRAD[case])
    for name, v in variants.items():
        _report('wgrad case %d' % case, name, np.abs(v - got).max() / gate)


# ==== 2. data gradient on stream-K =========================================================================================
def _dgrad_entries(L, _lib, fw, ctx, d, dzg, dzs, w_d, k, cin):
    """name -> (call(acc, dx, ws, ws_bytes), gate kind)."""
    ones, zeros = torch.ones(cin, device=dzg.device), torch.zeros(cin, device=dzg.device)

    def direct(acc, dx, ws, nb):
        _lib.check(L.y3_conv2d_dgrad(ctx, ctypes.byref(d), fw.ptr(dzg), dzs, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros), acc,
                                     fw.ptr(dx), fw.ptr(ws), ctypes.c_size_t(nb)))

    def split(planes):
        wsd = torch.empty(planes * k * k * cin * dzs, dtype=torch.bfloat16, device=dzg.device)
        _lib.check(L.y3_pack_conv_weights_split_dgrad(ctx, fw.ptr(w_d), k, cin, dzs, planes, fw.ptr(wsd)))

        def call(acc, dx, ws, nb):
            _lib.check(L.y3_conv2d_dgrad_split(ctx, ctypes.byref(d), planes, fw.ptr(dzg), dzs, fw.ptr(wsd), fw.ptr(ones),
                                               fw.ptr(zeros), acc, fw.ptr(dx), fw.ptr(ws), ctypes.c_size_t(nb)))
        return call
    return dict(direct=direct, split3=lambda: split(3), split2=lambda: split(2))


def _run_dgrad(call, want, prior, gate_kind, what):
    """accumulate 0 / 1, with and without the workspace; the runs with it twice.  Returns the accumulate = 1 stream-K result."""
    dev = prior.device
    prior_np = prior.cpu().numpy().astype(np.float64)
    kept = None
    for use_ws in (True, False):
        for acc in (0, 1):
            outs = []
            for _ in range(2 if use_ws else 1):
                dx = prior.clone() if acc else torch.full(want.shape, float('nan'), device=dev)
                ws = _nan_bytes(WS_BYTES) if use_ws else None
                call(acc, dx, ws, WS_BYTES if use_ws else 0)
                outs.append(dx)
            if use_ws:
                assert torch.equal(outs[0], outs[1]), '%s: stream-K runs differ (accumulate=%d)' % (what, acc)
            got = outs[0].cpu().numpy()
            ref = want + prior_np if acc else want
            name = '%s accumulate=%d workspace=%s' % (what, acc, use_ws)
            if gate_kind == 'elementwise':
                _check_elementwise(got, ref, name)
            else:
                _check_of_max(got, ref, 5e-3, name)
            if use_ws and acc:
                kept = got
    return kept


@functools.lru_cache(maxsize=None)
def _dgrad_s1_case(case):
    n, h, w, cin, cout = C.DGRAD_S1[case]
    rng = np.random.RandomState(200 + case)
    dz = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    return dz, wt, prior, dgrad64(dz, wt, (n, h, w, cin), 3, 1)


@pytest.mark.parametrize('entry', ['direct', 'split3', 'split2'])
@pytest.mark.parametrize('case', range(len(C.DGRAD_S1)))
def test_stride1_data_gradient_on_streamk(case, entry):
    fw, _lib, L, ctx = _ctx()
    n, h, w, cin, cout = C.DGRAD_S1[case]
    dzs = cout
    assert C.schedule(L, n, h, w, dzs, 0, cin, 3, 1, 0, 1) == C.STREAMK
    assert C.schedule(L, n, h, w, dzs, 0, cin, 3, 1, 0, 0) == C.ONE_PER_TILE
    dz, wt, prior, want = _dgrad_s1_case(case)
    d = C.desc(n, h, w, cin, 0, cout, 3, 1)
    dzg, w_d, pg = _gpu(dz), _gpu(wt.reshape(9 * cin, cout)), _gpu(prior)
    call = _dgrad_entries(L, _lib, fw, ctx, d, dzg, dzs, w_d, 3, cin)[entry]
    if entry != 'direct':
        call = call()
    got = _run_dgrad(call, want, pg, 'of_max' if entry == 'split2' else 'elementwise', entry)

    # ---- 5. guards ----
    if case != 0 or entry != 'direct':
        return
    ref = want + prior.astype(np.float64)
    gate = _elementwise_gate(ref)
    wm = np.zeros_like(wt)
    wm[1, 1, :, 32:64] = wt[1, 1, :, 32:64]                       # one K-step: the centre tap's second 32 dz channels
    delta = dgrad64(dz, wm, (n, h, w, cin), 3, 1).reshape(-1, cin)
    v = ref.reshape(-1, cin).copy()
    v[128:256, :128] -= delta[128:256, :128]                      # ... missing from the second 128x128 tile
    variants = {'kstep_dropped_from_one_tile': v.reshape(ref.shape), 'prior_added_twice': ref + prior}
    assert sorted(variants) == sorted(GUARDS_DGRAD_S1)
    for name, v in variants.items():
        _report('dgrad s1', name, (np.abs(v - got) / gate).max())


@functools.lru_cache(maxsize=None)
def _dgrad_s2_full():
    """The batch-4 case; the batch-2 case is its first two images (a conv's gradient is per image)."""
    n, h, w, cin, cout = 4, 90, 92, 128, 256
    rng = np.random.RandomState(300)
    dz = rng.standard_normal((n, h // 2, w // 2, cout)).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    return dz, wt, prior, dgrad64(dz, wt, (n, h, w, cin), 3, 2)


@pytest.mark.parametrize('case', range(len(C.DGRAD_S2)))
def test_stride2_data_gradient_parity_classes_on_streamk(case):
    """One call, four launches that share the workspace's flag words; at batch 2 the one-tap class stays data-parallel."""
    fw, _lib, L, ctx = _ctx()
    n, h, w, cin, cout, sched = C.DGRAD_S2[case]
    dzs = cout
    assert tuple(C.schedule(L, n, h // 2, w // 2, dzs, 0, cin, 3, 1, t, 1) for t in C.PARITY_TAPS) == sched
    assert all(C.schedule(L, n, h // 2, w // 2, dzs, 0, cin, 3, 1, t, 0) == C.ONE_PER_TILE for t in C.PARITY_TAPS)
    dz, wt, prior, want = _dgrad_s2_full()
    dz, prior, want = dz[:n], prior[:n], want[:n]
    d = C.desc(n, h, w, cin, 0, cout, 3, 2)
    dzg, w_d, pg = _gpu(dz), _gpu(wt.reshape(9 * cin, cout)), _gpu(prior)
    call = _dgrad_entries(L, _lib, fw, ctx, d, dzg, dzs, w_d, 3, cin)['direct']
    got = _run_dgrad(call, want, pg, 'elementwise', 'stride 2, batch %d' % n)

    # ---- 5. guards ----
    if case != 0:
        return
    ref = want + prior.astype(np.float64)
    gate = _elementwise_gate(ref)
    variants = {'prior_added_twice': ref + prior}
    # the pixels (even y, odd x; taps (1,0) and (1,2)) computed with the kernel transposed in space: the weights of the taps
    # (0,1) and (2,1), which belong to the (odd y, even x) class
    other = dgrad64(dz, np.ascontiguousarray(wt.transpose(1, 0, 2, 3)), (n, h, w, cin), 3, 2) + prior
    v = ref.copy()
    v[:, 0::2, 1::2] = other[:, 0::2, 1::2]
    variants['parity_class_with_anothers_taps'] = v
    # one K-step (one tap's 32 dz channels) missing from the first 128 x 128 tile of the four-tap class (odd y, odd x; input
    # row y meets output row o under tap ky where y = 2 o + ky - 1, so its taps are the kernel's corners): the tile's rows are
    # the class's first 128 pixels in row-major order
    wm = np.zeros_like(wt)
    wm[0, 0, :, 64:96] = wt[0, 0, :, 64:96]
    delta = dgrad64(dz[:1], wm, (1, h, w, cin), 3, 2)
    v = ref.copy()
    cls = v[0, 1::2, 1::2].reshape(-1, cin)                        # (a copy: written back below)
    cls[:128] -= delta[0, 1::2, 1::2].reshape(-1, cin)[:128]
    v[0, 1::2, 1::2] = cls.reshape(h // 2, w // 2, cin)
    assert np.abs(delta[0, 1::2, 1::2]).max() > 0
    variants['kstep_dropped_from_one_tile'] = v
    assert sorted(variants) == sorted(GUARDS_DGRAD_S2)
    for name, v in variants.items():
        _report('dgrad s2', name, (np.abs(v - got) / gate).max())


# ==== 3. the resident walk, forward =========================================================================================
def _pack(L, _lib, fw, ctx, wt):
    k, _, cin, cout = wt.shape
    wg = _gpu(wt)
    wp = torch.empty(k * k * cin * cout, device=wg.device)
    _lib.check(L.y3_pack_conv_weights(ctx, fw.ptr(wg), k, cin, cout, fw.ptr(wp)))
    return wp


@pytest.mark.parametrize('case', range(len(C.FWD)), ids=[c[0].replace(' ', '_') for c in C.FWD])
def test_forward_1x1_around_the_resident_walk(case):
    fw, _lib, L, ctx = _ctx()
    name, n, h, w, cin, c_up, cout, act, sched = C.FWD[case]
    assert C.schedule(L, n, h, w, cin, c_up, cout, 1, 1) == sched
    rng = np.random.RandomState(400 + case)
    x, wt, scale, shift = make_case(rng, n, h, w, 1, cin - c_up, cout)
    xu = None
    if c_up:
        xu = rng.standard_normal((n, h // 2, w // 2, c_up)).astype(np.float32)
        wt = (rng.standard_normal((1, 1, cin, cout)) * np.sqrt(2.0 / cin)).astype(np.float32)
    d = C.desc(n, h, w, cin, c_up, cout, 1, 1, act)
    wp = _pack(L, _lib, fw, ctx, wt)
    xg, sg, hg = _gpu(x), _gpu(scale), _gpu(shift)
    xug = None if xu is None else _gpu(xu)
    y = torch.full((n, h, w, cout), float('nan'), device=xg.device)
    _lib.check(L.y3_conv2d_fwd(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(xug), fw.ptr(wp), fw.ptr(sg), fw.ptr(hg), None,
                               fw.ptr(y), None, ctypes.c_size_t(0)))
    full = x if xu is None else np.concatenate([np.repeat(np.repeat(xu, 2, 1), 2, 2), x], axis=3)   # upsampled channels first
    fwd_check(y.cpu().numpy(), ref_conv(full, wt, scale, shift, 1, 1, act), name)


def test_forward_statistics_on_the_resident_walk():
    """y3_conv2d_fwd_stats where a workgroup walks several tiles: z bit-identical to the plain call, every block's partial
    sums those of ITS 64 rows of z as stored (within the bound of a 64-term fp32 sum taken in any order: (64 + 1) * 2^-24 *
    sum |terms|, one rounding of its own per square), and the finalised statistics as the separate pass gives them
    (rtol 2e-5, atol 2e-6: test_train_gpu.test_conv_epilogue_statistics_equal_the_separate_pass)."""
    fw, _lib, L, ctx = _ctx()
    n, h, w, cin, cout = C.FWD_STATS
    assert C.schedule(L, n, h, w, cin, 0, cout, 1, 1) == C.RESIDENT
    rng = np.random.RandomState(450)
    x, wt, _, _ = make_case(rng, n, h, w, 1, cin, cout)
    gamma, beta = _gpu(rng.uniform(0.5, 1.5, cout).astype(np.float32)), _gpu(rng.normal(0, 0.3, cout).astype(np.float32))
    d = C.desc(n, h, w, cin, 0, cout, 1, 1)
    nblk = L.y3_conv_stats_blocks(ctypes.byref(d), 0)
    rows = n * h * w
    assert nblk == rows // 64
    wp = _pack(L, _lib, fw, ctx, wt)
    xg = _gpu(x)
    ones, zeros = torch.ones(cout, device=xg.device), torch.zeros(cout, device=xg.device)
    z_plain = torch.full((rows, cout), float('nan'), device=xg.device)
    _lib.check(L.y3_conv2d_fwd(ctx, ctypes.byref(d), fw.ptr(xg), None, fw.ptr(wp), fw.ptr(ones), fw.ptr(zeros), None,
                               fw.ptr(z_plain), None, ctypes.c_size_t(0)))
    z = torch.full((rows, cout), float('nan'), device=xg.device)
    part = torch.full((nblk, 2, cout), float('nan'), device=xg.device)
    _lib.check(L.y3_conv2d_fwd_stats(ctx, ctypes.byref(d), fw.ptr(xg), fw.ptr(wp), fw.ptr(ones), fw.ptr(zeros), fw.ptr(z),
                                     fw.ptr(part), None, ctypes.c_size_t(0)))
    assert torch.equal(z, z_plain)
    z64 = z.cpu().numpy().astype(np.float64).reshape(nblk, 64, cout)
    got = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    for j, terms in enumerate((z64, z64 * z64)):
        bound = (64 + 1) * U * np.abs(terms).sum(1)
        err = np.abs(got[:, j] - terms.sum(1))
        assert (err <= bound).all(), 'sum of z^%d: worst ratio to the bound %.3f' % (j + 1, (err / bound).max())
    # a block's partial in its neighbour's row would be far outside: the blocks hold different pixels
    assert (np.abs(np.roll(got[:, 0], 1, 0) - z64.sum(1)) > (64 + 1) * U * np.abs(z64).sum(1)).mean() > 0.9
    st, st2 = torch.empty((4, cout), device=xg.device), torch.empty((4, cout), device=xg.device)
    _lib.check(L.y3_bn_train_stats_partials(ctx, fw.ptr(part), nblk, rows, cout, fw.ptr(gamma), fw.ptr(beta),
                                            ctypes.c_float(1e-5), ctypes.c_float(0.9), fw.ptr(st[0]), fw.ptr(st[1]),
                                            fw.ptr(st[2]), fw.ptr(st[3]), None, None))
    sc = torch.empty(L.y3_reduce_scratch_bytes(cout), dtype=torch.uint8, device=xg.device)
    _lib.check(L.y3_bn_train_stats(ctx, fw.ptr(z_plain), rows, cout, fw.ptr(gamma), fw.ptr(beta), ctypes.c_float(1e-5),
                                   ctypes.c_float(0.9), fw.ptr(st2[0]), fw.ptr(st2[1]), fw.ptr(st2[2]), fw.ptr(st2[3]), None,
                                   None, fw.ptr(sc)))
    np.testing.assert_allclose(st.cpu().numpy(), st2.cpu().numpy(), rtol=2e-5, atol=2e-6)


# ==== 4. the BN backward reduction in the 1x1 data gradient's epilogue ======================================================
def _leaky_bn_autograd(z, gamma, beta, mask, dy):
    """fp64 autograd through leaky(BN_train(z)) on the LeakyReLU branches `mask` names: d gamma, d beta, dz."""
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    u = (zt - zt.mean(0)) * gt / torch.sqrt(zt.var(0, unbiased=False) + 1e-5) + bt
    y = u * torch.tensor(np.where(mask, 1.0, 0.1))
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return gt.grad.numpy(), bt.grad.numpy(), zt.grad.numpy()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', range(len(C.DGRAD_BN)))
def test_fused_bn_backward_reduction(case, accumulate):
    fw, _lib, L, ctx = _ctx()
    n, h, w, cin, cout, dzs, bm, sched = C.DGRAD_BN[case]
    m = n * h * w
    d = C.desc(n, h, w, cin, 0, cout, 1, 1)
    assert C.schedule(L, n, h, w, dzs, 0, cin, 1, 1) == sched
    nblk = L.y3_conv_dgrad_bn_blocks(ctypes.byref(d))
    assert nblk == -(-m // bm)
    rng = np.random.RandomState(500 + case)
    z = (rng.standard_normal((m, cin)) * 2 + rng.standard_normal(cin)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.normal(0, 0.3, cin).astype(np.float32)
    dz = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    wt = (rng.standard_normal((1, 1, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((m, cin)).astype(np.float32)
    zg, gg, bg, pg = _gpu(z), _gpu(gamma), _gpu(beta), _gpu(prior)
    dev = zg.device
    # the BN layer's vectors as the train step hands them over: [4][cin] mean, inv_std, folded scale, folded shift
    vec = torch.full((4, cin), float('nan'), device=dev)
    sc = torch.empty(L.y3_bn_bwd_scratch_bytes(cin), dtype=torch.uint8, device=dev)
    _lib.check(L.y3_bn_train_stats(ctx, fw.ptr(zg), m, cin, fw.ptr(gg), fw.ptr(bg), ctypes.c_float(1e-5), ctypes.c_float(0.9),
                                   fw.ptr(vec[0]), fw.ptr(vec[1]), fw.ptr(vec[2]), fw.ptr(vec[3]), None, None, fw.ptr(sc)))
    mean, istd, scale, shift = vec.cpu().numpy()
    dzg = _gpu(_pad_lanes(rng, dz, dzs))
    w_d = torch.zeros((cin, dzs), device=dev)
    w_d[:, :cout] = _gpu(wt.reshape(cin, cout))
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    outs = []
    for _ in range(2):
        dx = pg.clone() if accumulate else torch.full((m, cin), float('nan'), device=dev)
        part = torch.full((nblk, 2, cin), float('nan'), device=dev)
        _lib.check(L.y3_conv2d_dgrad_bn(ctx, ctypes.byref(d), fw.ptr(dzg), dzs, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros),
                                        accumulate, fw.ptr(dx), fw.ptr(zg), fw.ptr(vec), fw.ptr(part)))
        outs.append((dx, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'not run-to-run bit-exact'
    dxg, partg = outs[0]
    # the plain entry writes the same dx, bit for bit
    dx_plain = pg.clone() if accumulate else torch.full((m, cin), float('nan'), device=dev)
    _lib.check(L.y3_conv2d_dgrad(ctx, ctypes.byref(d), fw.ptr(dzg), dzs, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros), accumulate,
                                 fw.ptr(dx_plain), None, ctypes.c_size_t(0)))
    assert torch.equal(dxg, dx_plain)

    # (a) dx
    p64 = prior.astype(np.float64) if accumulate else 0.0
    want = dgrad64(dz, wt, (m, cin), 1, 1) + p64
    got = dxg.cpu().numpy()
    _check_elementwise(got, want, 'dx')

    # (b) every block's two sums against fp64 sums over that block's rows of the dx the GPU stored.  The LeakyReLU branch as
    # the kernel takes it: fp32 z * scale, rounded, + shift (a separate multiply and add), so no element sits on an edge.
    mask = (z * scale + shift) > 0
    slope = np.where(mask, 1.0, np.float64(np.float32(0.1)))
    zhat = (z.astype(np.float64) - mean.astype(np.float64)) * istd.astype(np.float64)

    def block_sums(dx64, slope):
        g = dx64 * slope
        pad = nblk * bm - m
        t = np.stack([g, g * zhat], 0)
        t = np.concatenate([t, np.zeros((2, pad, cin))], 1).reshape(2, nblk, bm, cin)
        return t.sum(2).transpose(1, 0, 2), np.abs(t).sum(2).transpose(1, 0, 2)       # [nblk][2][cin]
    sums, mags = block_sums(got.astype(np.float64), slope)
    rows_in = np.minimum(bm, m - bm * np.arange(nblk)).reshape(nblk, 1, 1)
    bound = (rows_in + 3) * U * mags
    gotp = partg.cpu().numpy().astype(np.float64)
    assert np.isfinite(gotp).all()
    ratio = (np.abs(gotp - sums) / bound).max()
    print('fused reduction case %d accumulate=%d: worst ratio to the sequential-sum bound %.4f' % (case, accumulate, ratio))
    assert ratio <= GATE_B <= 1.0

    # (c) y3_bn_train_bwd_partials on those partials against y3_bn_train_bwd on the same dx, and both against fp64 autograd
    res = []
    for fused in (True, False):
        dgam, dbet = torch.full((cin,), float('nan'), device=dev), torch.full((cin,), float('nan'), device=dev)
        dzo = torch.full((m, cin), float('nan'), device=dev)
        if fused:
            _lib.check(L.y3_bn_train_bwd_partials(ctx, fw.ptr(zg), fw.ptr(dxg), fw.ptr(gg), fw.ptr(vec[2]), fw.ptr(vec[3]),
                                                  fw.ptr(vec[0]), fw.ptr(vec[1]), m, cin, fw.ptr(partg), nblk, fw.ptr(dgam),
                                                  fw.ptr(dbet), fw.ptr(dzo), fw.ptr(sc)))
        else:
            _lib.check(L.y3_bn_train_bwd(ctx, fw.ptr(zg), fw.ptr(dxg), fw.ptr(gg), fw.ptr(vec[2]), fw.ptr(vec[3]), fw.ptr(vec[0]),
                                         fw.ptr(vec[1]), m, cin, fw.ptr(dgam), fw.ptr(dbet), fw.ptr(dzo), fw.ptr(sc)))
        res.append([t.cpu().numpy().astype(np.float64) for t in (dgam, dbet, dzo)])
    wg, wb, wz = _leaky_bn_autograd(z, gamma, beta, mask, got)
    for name, r in zip(('fused', 'separate pass'), res):
        for what, a, b in zip(('d gamma', 'd beta', 'dz'), r, (wg, wb, wz)):
            _check_of_max(a, b, 2e-4, '%s: %s' % (name, what))
    # the two routes differ by the rounding of their fp32 partial sums only (combined in fp64 in both).  Per column that is at
    # most (bm + 3) * u * sum |terms| for the epilogue's blocks and (m + 3) * u * sum |terms| for the separate pass, whatever
    # rows its blocks take; d gamma carries inv_std.  dz moves by gamma * inv_std * (|d dbeta| + |zhat| |d dgamma|) / m, plus
    # a few roundings of the apply pass.
    tot = mags.sum(0)                                            # [2][cin]: sum |g'|, sum |g' zhat| over all rows
    tol_b = ((bm + 3) + (m + 3)) * U * tot[0] + 2 * U * np.abs(wb)
    tol_g = ((bm + 3) + (m + 3)) * U * tot[1] + 2 * U * np.abs(wg)
    assert (np.abs(res[0][1] - res[1][1]) <= tol_b).all()
    assert (np.abs(res[0][0] - res[1][0]) <= tol_g).all()
    tol_z = np.abs(gamma * istd) * (tol_b + np.abs(zhat).max(0) * tol_g) / m + 8 * U * np.abs(wz).max()
    assert (np.abs(res[0][2] - res[1][2]) <= tol_z).all()

    # ---- 5. guards: distances in gates of (a) and (b) ----
    gate_b = GATE_B * bound
    dist_b = lambda s: (np.abs(s - gotp) / gate_b).max()
    if accumulate:
        _report('fused bn case %d' % case, 'prior_added_twice', (np.abs(want + prior - got) / _elementwise_gate(want)).max())
        _report('fused bn case %d' % case, 'prior_left_out_of_g', dist_b(block_sums(got.astype(np.float64) - prior, slope)[0]))
    _report('fused bn case %d' % case, 'partial_written_to_next_block', dist_b(np.roll(sums, 1, 0)))
    _report('fused bn case %d' % case, 'partial_written_to_previous_block', dist_b(np.roll(sums, -1, 0)))
    u64 = z.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    flips = int(((u64 > 0) != mask).sum())
    if flips == 0:
        print('guard fused bn case %d: mask_from_fp64_u is vacuous here (no element of %d changes branch)' % (case, mask.size))
    else:
        s64 = block_sums(got.astype(np.float64), np.where(u64 > 0, 1.0, np.float64(np.float32(0.1))))[0]
        print('guard fused bn case %d: mask_from_fp64_u flips %d elements, %.1f gates' % (case, flips, dist_b(s64)))


def test_fused_bn_backward_reduction_refuses_what_it_cannot_take():
    """(d) a 3x3, a stride-2 and a fused-upsample desc, and null pointers: Y3_EINVAL, nothing written."""
    fw, _lib, L, ctx = _ctx()
    n, h, w, cin, cout = 2, 8, 8, 64, 64
    dev = fw.default_device()
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    dzg, w_d, zg, vec = torch.zeros((n * h * w, cout), device=dev), torch.zeros((9 * cin, cout), device=dev), \
        torch.zeros((n * h * w, cin), device=dev), torch.ones((4, cin), device=dev)
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    dx, part = nan(n * h * w, cin), nan(n * h * w, 2, cin)
    for bad in (C.desc(n, h, w, cin, 0, cout, 3, 1), C.desc(n, h, w, cin, 0, cout, 3, 2), C.desc(n, h, w, cin, 32, cout, 1, 1)):
        assert L.y3_conv_dgrad_bn_blocks(ctypes.byref(bad)) == 0
        with pytest.raises(ValueError):
            _lib.check(L.y3_conv2d_dgrad_bn(ctx, ctypes.byref(bad), fw.ptr(dzg), cout, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros), 0,
                                            fw.ptr(dx), fw.ptr(zg), fw.ptr(vec), fw.ptr(part)))
    good = C.desc(n, h, w, cin, 0, cout, 1, 1)
    assert L.y3_conv_dgrad_bn_blocks(ctypes.byref(good)) == 1
    args = [fw.ptr(dzg), cout, fw.ptr(w_d), fw.ptr(ones), fw.ptr(zeros), 0, fw.ptr(dx), fw.ptr(zg), fw.ptr(vec), fw.ptr(part)]
    for i in (0, 2, 3, 4, 6, 7, 8, 9):
        a = list(args)
        a[i] = None
        with pytest.raises(ValueError):
            _lib.check(L.y3_conv2d_dgrad_bn(ctx, ctypes.byref(good), *a))
    with pytest.raises(ValueError):
        _lib.check(L.y3_conv2d_dgrad_bn(ctx, None, *args))
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and torch.isnan(part).all()
