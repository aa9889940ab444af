"""Guard-band tests: no public entry point that takes a device pointer touches a byte outside the buffers it was handed
(include/yolo355.h, Conventions).

Table-driven: one Entry = the entry points it calls (`covers`) and one small case.  Its builder returns a Run:
  specs    the tensors, as guarded.Spec: name, role, data, alignment.  Every tensor sits at EXACTLY that alignment (16 bytes
           unless the header documents another) between two poisoned guards of at least 1 MiB; a scratch / workspace has exactly
           the bytes its size function returned (S(...) below);
  call     a closure over the arena's tensors that calls _lib.lib().y3_* directly;
  outputs  the tensors kept from each pass;
  verify   the reference, at the tolerance the op's own parity test uses (named in the builder; no tolerance is new here).
test_guard_bands runs the case twice (guards, outputs and scratch poisoned with 0xFF = NaN, then with 0x7F = 3.4e38), asserts
after each pass that no guard byte changed, that the two passes' outputs are bit-identical, and that they match the reference.
test_every_entry_point_is_covered_or_excluded (no GPU) holds the table against _lib.PROTOTYPES."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
from guarded import Spec
from conftest import COCO_ANCHORS
import conv_schedule_cases as C
import test_conv_gpu as TC
import test_conv_schedules_gpu as TS
import test_conv_ranges_gpu as TR
import test_bf16_gpu as TB
import test_train_bf16_kernels_gpu as TK
import test_train_gpu as TT
import test_optimizer_gpu as TO
import test_loss_gpu as TL
import test_decode_gpu as TD
import voc_cases as vc
import coco_cases as cc
import beval_cases as bc
from device_eval_helpers import nms_like

F32, BF16, F64, I32, I64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8
U = 2.0 ** -24

# Entry points with a pointer argument that the table leaves out, each with its reason.
EXCLUDED = {
    # the issue's exclusions
    'y3_jpeg_decode': 'takes a byte blob with its size and checks every record against it before anything is launched',
    'y3_feed_run': 'takes a byte blob with its size and checks every record against it before anything is launched',
    # the data-parallel path: hooks of the RCCL train step, no kernel of their own
    'y3_net_train_set_wgrad_stream': 'data-parallel / second-stream plumbing: takes a stream handle, launches nothing',
    'y3_net_train_set_bn_sync': 'data-parallel path (the exchange buffer belongs to the RCCL step)',
    # context, net-handle and host-pointer-only functions
    'y3_ctx_create': 'context', 'y3_ctx_destroy': 'context', 'y3_ctx_check': 'context',
    'y3_net_create': 'net handle', 'y3_net_destroy': 'net handle', 'y3_net_num_layers': 'net handle',
    'y3_net_layer_info': 'net handle, host pointers', 'y3_net_params_bytes': 'net handle', 'y3_net_workspace_bytes': 'net handle',
    'y3_net_layer_graph': 'net handle, host pointers', 'y3_net_num_tensors': 'net handle',
    'y3_net_tensor_info': 'net handle, host pointers', 'y3_net_set_dtype': 'net handle', 'y3_net_set_profiling': 'net handle',
    'y3_net_get_layer_ms': 'net handle, host pointer', 'y3_net_layer_is_streamk': 'net handle', 'y3_net_layer_fused': 'net handle',
    'y3_net_train_workspace_bytes': 'net handle, host table', 'y3_net_train_saved': 'net handle, host pointers',
    'y3_net_train_saved_type': 'net handle',
    'y3_conv_workspace_bytes': 'host pointer only', 'y3_streamk_range': 'host pointers only', 'y3_conv_image_ranges': 'host pointers only',
    'y3_conv_wino_eligible': 'host pointer only', 'y3_conv_wino_workspace_bytes': 'host pointer only',
    'y3_conv_wino44_eligible': 'host pointer only', 'y3_conv_wino44_candidate': 'host pointer only',
    'y3_conv_wino44_preferred': 'host pointer only', 'y3_conv_wino44_workspace_bytes': 'host pointer only',
    'y3_conv_bf16_tile': 'host pointer only', 'y3_conv_train_stats_blocks_bf16': 'host pointer only',
    'y3_conv_wgrad_bf16_scratch_bytes': 'host pointer only', 'y3_conv_stats_blocks': 'host pointer only',
    'y3_conv_dgrad_bn_blocks': 'host pointer only', 'y3_conv_schedule': 'host pointer only',
    'y3_conv_wgrad_scratch_bytes': 'host pointer only', 'y3_conv_wgrad_wino_eligible': 'host pointer only',
    'y3_conv_wgrad_wino_scratch_bytes': 'host pointer only', 'y3_clip_update_multi_scratch_bytes': 'host pointer only',
}

Run = collections.namedtuple('Run', 'specs call outputs verify view')
Entry = collections.namedtuple('Entry', 'id covers build')
TABLE = []


def entry(id_, covers, build, *args, **kw):
    TABLE.append(Entry(id_, tuple(covers), lambda g: build(g, *args, **kw)))


def run_of(specs, call, outputs, verify, view=None):
    return Run(specs, call, outputs, verify, view)


class G(object):
    """The library, the context of torch's current stream, and the record of which entry points a case called."""

    def __init__(self):
        from yolov3_tensorflow_amd import framework as fw, _lib
        self.fw, self._lib, self.L, self.dev = fw, _lib, _lib.lib(), fw.default_device()
        self.ctx = fw.context()
        self.called = set()

    def __call__(self, name, *args):
        self.called.add(name)
        self._lib.check(getattr(self.L, name)(*args))


def P(t):
    """device pointer of an arena tensor; NULL for None and for a zero-byte scratch"""
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def S(name, nbytes, align=16):
    """scratch / workspace of exactly `nbytes` (what the size function returned)"""
    return Spec(name, 'scratch', shape=(int(nbytes),), dtype=U8, align=align)


def IN(name, data, align=16, dtype=None):
    return Spec(name, 'in', data=data if dtype is None else torch.as_tensor(np.asarray(data)).to(dtype), align=align)


def INOUT(name, data, align=16):
    return Spec(name, 'inout', data=data, align=align)


def OUT(name, shape, dtype=F32, align=16):
    return Spec(name, 'out', shape=shape, dtype=dtype, align=align)


def opt(fn, *a):
    return fn(*a) if a[-1] is not None else None


def cf(x):
    return ctypes.c_float(x)


def host_f32(a):
    """a HOST array of floats for the anchors arguments (owns its memory)"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return (ctypes.c_float * a.size)(*a.tolist())


def npf(t):
    return t.float().numpy() if t.dtype == BF16 else t.numpy()


def rel_err(got, want):
    return TT.rel_err(np.asarray(got, np.float64), np.asarray(want, np.float64))


# ============================================================================================================================
# fp32 inference convs.  Reference: test_conv_gpu.ref_conv (fp64); tolerance: test_conv_gpu.check (1e-4 * (1 + |ref|); the
# two-plane split 2e-3).  The packers run inside the call: their output is a guarded 'out' tensor the conv then reads.
# ============================================================================================================================
@functools.lru_cache(maxsize=None)
def _conv_case(n, h, w, k, stride, cin, cout, act, resid, c_up):
    rng = np.random.RandomState(n * 1000 + h * 10 + cin + cout + k)
    x, wt, scale, shift = TC.make_case(rng, n, h, w, k, cin - c_up, cout)
    xu = None
    if c_up:
        xu = rng.standard_normal((n, h // 2, w // 2, c_up)).astype(np.float32)
        wt = (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
    r = rng.standard_normal((n, h // stride, w // stride, cout)).astype(np.float32) if resid else None
    full = x if xu is None else np.concatenate([np.repeat(np.repeat(xu, 2, 1), 2, 2), x], axis=3)
    want = TC.ref_conv(full, wt, scale, shift, k, stride, act, r)
    return x, xu, wt, scale, shift, r, want


def conv_fwd(g, shape, form='direct', ws='null', stats=False):
    """form: 'direct' | 'split2' | 'split3' | 'wino' | 'wino44'.  ws: 'null' (workspace = NULL) or 'exact' (exactly the bytes of
    the form's size function).  stats: the training entry (*_stats) followed by y3_bn_train_stats_partials."""
    n, h, w, k, stride, cin, cout, act, resid, c_up = shape
    x, xu, wt, scale, shift, r, want = _conv_case(*shape)
    L = g.L
    d = C.desc(n, h, w, cin, c_up, cout, k, stride, act)
    planes = {'split2': 2, 'split3': 3}.get(form, 0)
    size_fn = {'wino': L.y3_conv_wino_workspace_bytes, 'wino44': L.y3_conv_wino44_workspace_bytes}.get(form, L.y3_conv_workspace_bytes)
    wsb = size_fn(ctypes.byref(d)) if ws == 'exact' else 0
    if ws == 'exact':
        assert wsb > 0, 'this case exists for a non-zero workspace'
        if form in ('direct', 'split2', 'split3'):
            assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) == C.STREAMK and L.y3_conv_schedule(ctypes.byref(d), 0, 0) == C.ONE_PER_TILE
    ho, wo = h // stride, w // stride
    if cin == 3:
        wp = None
    elif planes:
        wp = OUT('w_packed', (planes * k * k * cin * cout,), BF16)
    else:
        wp = OUT('w_packed', ({'wino': 16, 'wino44': 36}.get(form, k * k) * cin * cout,))
    nblk = L.y3_conv_stats_blocks(ctypes.byref(d), {'wino': 1, 'wino44': 2}.get(form, 0)) if stats else 0
    rng = np.random.RandomState(7)
    gamma, beta = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.3, cout).astype(np.float32)
    specs = [IN('x', x), opt(IN, 'x_up', xu), IN('w_hwio', wt), wp, IN('scale', scale), IN('shift', shift), opt(IN, 'residual', r),
             OUT('y', (n, ho, wo, cout)), S('workspace', wsb)]
    if stats:
        assert nblk > 0 and r is None and xu is None
        specs += [OUT('stats', (nblk, 2, cout)), IN('gamma', gamma), IN('beta', beta), OUT('bn', (4, cout)),
                  INOUT('moving_mean', np.full(cout, 0.25, np.float32)), INOUT('moving_var', np.full(cout, 2.0, np.float32))]

    def call(a):
        ctx, D = g.ctx, ctypes.byref(d)
        t = lambda name: P(a[name]) if name in [s.name for s in a.slots] else None
        wsz = ctypes.c_size_t(wsb)
        if form == 'direct':
            if cin != 3:
                g('y3_pack_conv_weights', ctx, t('w_hwio'), k, cin, cout, t('w_packed'))
            wk = t('w_packed') if cin != 3 else t('w_hwio')
            if stats:
                g('y3_conv2d_fwd_stats', ctx, D, t('x'), wk, t('scale'), t('shift'), t('y'), t('stats'), t('workspace'), wsz)
            else:
                g('y3_conv2d_fwd', ctx, D, t('x'), t('x_up'), wk, t('scale'), t('shift'), t('residual'), t('y'), t('workspace'), wsz)
        elif planes:
            g('y3_pack_conv_weights_split', ctx, t('w_hwio'), k, cin, cout, planes, t('w_packed'))
            g('y3_conv2d_fwd_split', ctx, D, planes, t('x'), t('x_up'), t('w_packed'), t('scale'), t('shift'), t('residual'), t('y'),
              t('workspace'), wsz)
        else:
            sfx = '_' + form
            g('y3_pack_conv_weights' + sfx, ctx, t('w_hwio'), cin, cout, t('w_packed'))
            if stats:
                g('y3_conv2d_fwd%s_stats' % sfx, ctx, D, t('x'), t('w_packed'), t('scale'), t('shift'), t('y'), t('stats'),
                  t('workspace'), wsz)
            else:
                g('y3_conv2d_fwd' + sfx, ctx, D, t('x'), t('w_packed'), t('scale'), t('shift'), t('residual'), t('y'), t('workspace'), wsz)
        if stats:
            bn = a['bn']
            g('y3_bn_train_stats_partials', ctx, t('stats'), nblk, n * ho * wo, cout, t('gamma'), t('beta'), cf(1e-5), cf(0.9),
              P(bn[0]), P(bn[1]), P(bn[2]), P(bn[3]), t('moving_mean'), t('moving_var'))

    def verify(o):
        TC.check(o['y'].numpy(), want, '%s %s' % (form, shape), planes)
        if stats:
            check_bn_statistics(o['y'].numpy().reshape(-1, cout), gamma, beta, o['bn'].numpy(), o['moving_mean'].numpy(),
                                o['moving_var'].numpy())

    outs = ['y'] + (['w_packed'] if wp is not None else []) + (['stats', 'bn', 'moving_mean', 'moving_var'] if stats else [])
    return run_of(specs, call, outs, verify)


def check_bn_statistics(z, gamma, beta, bn, mm, mv):
    """mean / inv_std / scale / shift / moving statistics of z [rows][c] (as stored) against fp64, at the tolerances of
    test_train_gpu.py: mean 1e-5 of max|z| (test_conv_epilogue_statistics_equal_the_separate_pass), inv_std, scale and shift
    rtol 2e-5 (test_bn_train_stats_and_apply_without_moving_statistics_or_residual), moving statistics rtol 1e-5 / atol 1e-6
    (test_bn_train_forward_backward)."""
    z = z.astype(np.float64)
    rows = z.shape[0]
    mean, var = z.mean(0), z.var(0)
    inv_std = 1.0 / np.sqrt(var + 1e-5)
    scale = gamma.astype(np.float64) * inv_std
    shift = beta.astype(np.float64) - mean * scale
    assert np.abs(bn[0] - mean).max() <= 1e-5 * np.abs(z).max()
    np.testing.assert_allclose(bn[1], inv_std, rtol=2e-5)
    np.testing.assert_allclose(bn[2], scale, rtol=2e-5)
    np.testing.assert_allclose(bn[3], shift, rtol=2e-5, atol=2e-5 * float(np.abs(mean * scale).max()))
    if mm is not None:
        np.testing.assert_allclose(mm, 0.25 * 0.9 + mean * 0.1, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(mv, 2.0 * 0.9 + var * rows / (rows - 1.0) * 0.1, rtol=1e-5, atol=1e-6)


# (n, h, w, k, stride, cin, cout, act, residual, c_up)
CONV_SHAPES = collections.OrderedDict([
    ('3x3s1_res', (3, 10, 14, 3, 1, 32, 64, 1, True, 0)),
    ('3x3s2', (3, 10, 14, 3, 2, 32, 64, 1, False, 0)),           # M = 105
    ('1x1', (3, 10, 14, 1, 1, 64, 32, 1, False, 0)),
    ('head255', (1, 13, 13, 1, 1, 1024, 255, 0, False, 0)),
    ('head18', (1, 13, 13, 1, 1, 1024, 18, 0, False, 0)),
    ('small_map', (5, 2, 2, 3, 1, 64, 64, 1, False, 0)),         # map smaller than the kernel footprint
    ('upcat', (2, 6, 10, 1, 1, 64, 64, 1, False, 32)),           # c_up 32 + 32 route channels
    ('streamk', (7, 26, 26, 3, 1, 64, 1024, 1, True, 0)),        # 19 x 8 tiles of 128 x 128; the existing tests' stream-K case
])
STEM = (1, 12, 20, 3, 1, 3, 32, 1, False, 0)
WINO_SHAPES = collections.OrderedDict([
    ('5x3x5', (5, 3, 5, 3, 1, 64, 64, 0, False, 0)),
    ('1x2x2_c96', (1, 2, 2, 3, 1, 96, 64, 1, False, 0)),
    ('3x20x28_res', (3, 20, 28, 3, 1, 64, 128, 1, True, 0)),
    ('2x13x13', (2, 13, 13, 3, 1, 64, 128, 1, False, 0)),
])
WINO44_ONLY = collections.OrderedDict([
    ('7x13x13_c160', (7, 13, 13, 3, 1, 160, 64, 1, True, 0)),
    ('1x9x130', (1, 9, 130, 3, 1, 32, 192, 1, True, 0)),
])
for _name, _shape in CONV_SHAPES.items():
    entry('conv_fwd-%s-null' % _name, ('y3_pack_conv_weights', 'y3_conv2d_fwd'), conv_fwd, _shape)
    for _p in (3, 2):
        entry('conv_fwd_split%d-%s-null' % (_p, _name), ('y3_pack_conv_weights_split', 'y3_conv2d_fwd_split'), conv_fwd, _shape,
              form='split%d' % _p)
entry('conv_fwd-stem-null', ('y3_conv2d_fwd',), conv_fwd, STEM)
entry('conv_fwd-streamk-exact', ('y3_pack_conv_weights', 'y3_conv2d_fwd'), conv_fwd, CONV_SHAPES['streamk'], ws='exact')
for _p in (3, 2):
    entry('conv_fwd_split%d-streamk-exact' % _p, ('y3_pack_conv_weights_split', 'y3_conv2d_fwd_split'), conv_fwd,
          CONV_SHAPES['streamk'], form='split%d' % _p, ws='exact')
for _name, _shape in WINO_SHAPES.items():
    entry('conv_fwd_wino-%s-null' % _name, ('y3_pack_conv_weights_wino', 'y3_conv2d_fwd_wino'), conv_fwd, _shape, form='wino')
# 304 blocks on 256 workers: the F(2x2) kernel's stream-K schedule (test_conv_gpu.WINO_CASES), with and without its workspace
entry('conv_fwd_wino-streamk-null', ('y3_pack_conv_weights_wino', 'y3_conv2d_fwd_wino'), conv_fwd, CONV_SHAPES['streamk'], form='wino')
entry('conv_fwd_wino-streamk-exact', ('y3_pack_conv_weights_wino', 'y3_conv2d_fwd_wino'), conv_fwd, CONV_SHAPES['streamk'],
      form='wino', ws='exact')
for _name, _shape in list(WINO_SHAPES.items()) + list(WINO44_ONLY.items()):
    for _ws in ('null', 'exact'):               # the one-kernel form, and the two-kernel form on exactly the bytes of V
        entry('conv_fwd_wino44-%s-%s' % (_name, _ws), ('y3_pack_conv_weights_wino44', 'y3_conv2d_fwd_wino44'), conv_fwd, _shape,
              form='wino44', ws=_ws)
# the training entries: the conv with the column sums in its epilogue, finished by y3_bn_train_stats_partials
STATS_SHAPES = [('1x1_128x64', (3, 20, 28, 1, 1, 128, 64, 0, False, 0)), ('3x3s2', (2, 26, 26, 3, 2, 64, 128, 0, False, 0)),
                ('1x1_128x32', (2, 24, 24, 1, 1, 64, 32, 0, False, 0))]
for _name, _shape in STATS_SHAPES:
    entry('conv_fwd_stats-%s' % _name, ('y3_pack_conv_weights', 'y3_conv2d_fwd_stats', 'y3_bn_train_stats_partials'), conv_fwd, _shape,
          stats=True)
_ODD = (3, 13, 13, 3, 1, 64, 128, 0, False, 0)      # odd map: outputs that do not exist must not be counted
entry('conv_fwd_wino_stats-3x13x13', ('y3_pack_conv_weights_wino', 'y3_conv2d_fwd_wino_stats', 'y3_bn_train_stats_partials'), conv_fwd,
      _ODD, form='wino', stats=True)
for _ws in ('null', 'exact'):
    entry('conv_fwd_wino44_stats-3x13x13-%s' % _ws,
          ('y3_pack_conv_weights_wino44', 'y3_conv2d_fwd_wino44_stats', 'y3_bn_train_stats_partials'), conv_fwd, _ODD, form='wino44',
          ws=_ws, stats=True)


def stem_s2(g, n, h, w, bf16):
    """y3_conv2d_fwd_stem_s2 / y3_conv2d_fwd_bf16_stem_s2: test_conv_gpu.test_fused_stem_and_stride2_conv (check) and
    test_bf16_gpu.test_bf16_fused_stem_and_stride2_conv (2^-7 |ref| + 2e-2)."""
    rng = np.random.RandomState(h * 7 + w)
    if bf16:
        x = TB.bf16_round(rng.uniform(0, 1, (n, h, w, 3)))
        w0 = TB.bf16_round(rng.standard_normal((3, 3, 3, 32)) * np.sqrt(2.0 / 27))
        w1 = TB.bf16_round(rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / 288))
        sc0, sh0 = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.normal(0, 0.2, 32).astype(np.float32)
        sc1, sh1 = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
        want = TB.ref_conv(TB.bf16_round(TB.ref_conv(x, w0, sc0, sh0, 3, 1, True)), w1, sc1, sh1, 3, 2, True)
    else:
        x = rng.uniform(0, 1, (n, h, w, 3)).astype(np.float32)
        _, w0, sc0, sh0 = TC.make_case(rng, 1, 1, 1, 3, 3, 32)
        _, w1, sc1, sh1 = TC.make_case(rng, 1, 1, 1, 3, 32, 64)
        want = TC.ref_conv(TC.ref_conv(x, w0, sc0, sh0, 3, 1, True).astype(np.float64), w1, sc1, sh1, 3, 2, True)
    specs = [IN('x', x), IN('w0_hwio', w0), IN('scale0', sc0), IN('shift0', sh0), IN('w1_hwio', w1),
             OUT('w1_packed', (9 * 64 * 32,), BF16 if bf16 else F32), IN('scale1', sc1), IN('shift1', sh1),
             OUT('y', (n, h // 2, w // 2, 64), BF16 if bf16 else F32)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_pack_conv_weights_bf16' if bf16 else 'y3_pack_conv_weights', g.ctx, t('w1_hwio'), 3, 32, 64, t('w1_packed'))
        g('y3_conv2d_fwd_bf16_stem_s2' if bf16 else 'y3_conv2d_fwd_stem_s2', g.ctx, n, h, w, t('x'), t('w0_hwio'), t('scale0'),
          t('shift0'), t('w1_packed'), t('scale1'), t('shift1'), t('y'))

    def verify(o):
        got = npf(o['y'])
        if bf16:
            assert np.isfinite(got).all() and (np.abs(got - want) <= 2.0 ** -7 * np.abs(want) + 2e-2).all()
        else:
            TC.check(got, want, 'fused stem + stride-2 conv')
    return run_of(specs, call, ['y', 'w1_packed'], verify)


entry('conv_fwd_stem_s2-1x70x38', ('y3_pack_conv_weights', 'y3_conv2d_fwd_stem_s2'), stem_s2, 1, 70, 38, False)


# ============================================================================================================================
# bf16 inference.  Reference and tolerance: test_bf16_gpu.py (fp64 conv of the same bf16-rounded operands; (1e-4 if the output
# is fp32 else 2^-8) * |ref| + 2e-3; the fused kernels 2^-7 |ref| + 2e-2).
# ============================================================================================================================
def conv_bf16(g, n, h, w, k, stride, cin, cout, resid, c_up, out_f32):
    rng = np.random.RandomState(cin * 7 + cout)
    x = TB.bf16_round(rng.standard_normal((n, h, w, cin - c_up)))
    xu = TB.bf16_round(rng.standard_normal((n, h // 2, w // 2, c_up))) if c_up else None
    wt = TB.bf16_round(rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (k * k * cin)))
    scale, shift = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.2, cout).astype(np.float32)
    ho, wo = h // stride, w // stride
    r = TB.bf16_round(rng.standard_normal((n, ho, wo, cout))) if resid else None
    xin = x if xu is None else np.concatenate([np.repeat(np.repeat(xu, 2, 1), 2, 2), x], axis=3)
    want = TB.ref_conv(xin, wt, scale, shift, k, stride, not out_f32, r)
    d = C.desc(n, h, w, cin, c_up, cout, k, stride, 0 if out_f32 else 1)
    b = lambda name, v: None if v is None else IN(name, v, dtype=BF16)
    specs = [b('x', x), b('x_up', xu), IN('w_hwio', wt), OUT('w_packed', (k * k * cin * cout,), BF16), IN('scale', scale),
             IN('shift', shift), b('residual', r), OUT('y', (n, ho, wo, cout), F32 if out_f32 else BF16)]

    def call(a):
        t = lambda name: P(a[name]) if name in [s.name for s in a.slots] else None
        g('y3_pack_conv_weights_bf16', g.ctx, t('w_hwio'), k, cin, cout, t('w_packed'))
        g('y3_conv2d_fwd_bf16', g.ctx, ctypes.byref(d), t('x'), t('x_up'), t('w_packed'), t('scale'), t('shift'), t('residual'), t('y'),
          out_f32)

    def verify(o):
        got = npf(o['y'])
        assert np.isfinite(got).all()
        assert (np.abs(got - want) <= (1e-4 if out_f32 else 2.0 ** -8) * np.abs(want) + 2e-3).all(), float(np.abs(got - want).max())
    return run_of(specs, call, ['y', 'w_packed'], verify)


for _id, _a in [('3x3s1_res', (3, 20, 28, 3, 1, 32, 64, True, 0, 0)), ('3x3s2', (2, 26, 26, 3, 2, 64, 128, False, 0, 0)),
                ('1x1_c100', (2, 13, 17, 1, 1, 128, 100, False, 0, 0)), ('1x1_c255_f32_res', (2, 13, 17, 1, 1, 128, 255, True, 0, 1)),
                ('1x1_c136_res', (3, 21, 27, 1, 1, 192, 136, True, 0, 0)), ('1x1_upcat', (2, 26, 26, 1, 1, 384, 128, False, 128, 0)),
                ('1x1_ring', (1, 19, 19, 1, 1, 1024, 512, False, 0, 0))]:
    entry('conv_fwd_bf16-' + _id, ('y3_pack_conv_weights_bf16', 'y3_conv2d_fwd_bf16'), conv_bf16, *_a)
entry('conv_fwd_bf16_stem_s2-1x70x38', ('y3_pack_conv_weights_bf16', 'y3_conv2d_fwd_bf16_stem_s2'), stem_s2, 1, 70, 38, True)


def resblock_bf16(g, n, h, w):
    rng = np.random.RandomState(h * 5 + w)
    x = TB.bf16_round(rng.standard_normal((n, h, w, 64)))
    w2 = TB.bf16_round(rng.standard_normal((1, 1, 64, 32)) * np.sqrt(2.0 / 64))
    w3 = TB.bf16_round(rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / 288))
    sc2, sh2 = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.normal(0, 0.2, 32).astype(np.float32)
    sc3, sh3 = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
    want = TB.ref_conv(TB.bf16_round(TB.ref_conv(x, w2, sc2, sh2, 1, 1, True)), w3, sc3, sh3, 3, 1, True, x)
    specs = [IN('x', x, dtype=BF16), IN('w2_hwio', w2), IN('w3_hwio', w3), OUT('w2_packed', (64 * 32,), BF16),
             OUT('w3_packed', (9 * 64 * 32,), BF16), IN('scale2', sc2), IN('shift2', sh2), IN('scale3', sc3), IN('shift3', sh3),
             OUT('y', (n, h, w, 64), BF16)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_pack_conv_weights_bf16', g.ctx, t('w2_hwio'), 1, 64, 32, t('w2_packed'))
        g('y3_pack_conv_weights_bf16', g.ctx, t('w3_hwio'), 3, 32, 64, t('w3_packed'))
        g('y3_resblock64_fwd_bf16', g.ctx, n, h, w, t('x'), t('w2_packed'), t('scale2'), t('shift2'), t('w3_packed'), t('scale3'),
          t('shift3'), t('y'))

    def verify(o):
        got = npf(o['y'])
        assert np.isfinite(got).all() and (np.abs(got - want) <= 2.0 ** -7 * np.abs(want) + 2e-2).all()
    return run_of(specs, call, ['y', 'w2_packed', 'w3_packed'], verify)


entry('resblock64_fwd_bf16-1x35x19', ('y3_pack_conv_weights_bf16', 'y3_resblock64_fwd_bf16'), resblock_bf16, 1, 35, 19)


# ============================================================================================================================
# fp32 gradients.  Every dz has rows wider than cout (dz_stride > cout), the lanes behind cout holding finite junk.
# References: test_conv_schedules_gpu.dgrad64 / wgrad64 (fp64).  Tolerances: data gradient, exact kernel and three-plane split,
# elementwise 1e-4 * (1 + |ref|) (test_conv_schedules_gpu); two-plane split 5e-3 of max; Winograd forms 2e-4 of max
# (test_train_gpu); weight gradient 2e-4 of max.
# ============================================================================================================================
def _wider(cout):
    s = (cout + 31) // 32 * 32
    return s if s > cout else s + 32


@functools.lru_cache(maxsize=None)
def _grad_case(n, h, w, k, stride, cin, cout):
    rng = np.random.RandomState(cin + 3 * cout + k + h)
    ho, wo = h // stride, w // stride
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    dz = rng.standard_normal((n, ho, wo, cout)).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    dzs = cout if cin == 3 else _wider(cout)      # (the stem's weight gradient takes dz_stride = cout = 32 only)
    dzp = TS._pad_lanes(rng, dz, dzs)
    w_d = np.zeros((k * k * cin, dzs), np.float32)
    w_d[:, :cout] = wt.reshape(k * k * cin, cout)
    return x, dz, dzp, dzs, wt, w_d, prior


@functools.lru_cache(maxsize=None)
def _dgrad_ref(n, h, w, k, stride, cin, cout):
    x, dz, dzp, dzs, wt, w_d, prior = _grad_case(n, h, w, k, stride, cin, cout)
    return TS.dgrad64(dz, wt, (n, h, w, cin), k, stride)


@functools.lru_cache(maxsize=None)
def _wgrad_ref(n, h, w, k, stride, cin, cout):
    x, dz, dzp, dzs, wt, w_d, prior = _grad_case(n, h, w, k, stride, cin, cout)
    return TS.wgrad64(x, dz, k, stride)


def dgrad(g, shape, form, acc, ws='null', expect_streamk=False):
    """form: 'direct' | 'split3' | 'split2' | 'wino' | 'wino44'.  ws 'exact': the workspace of the conv as launched
    ([n, h/s, w/s, dz_stride] -> cin at stride 1): y3_conv_workspace_bytes / _wino_ / _wino44_workspace_bytes of that conv."""
    n, h, w, k, stride, cin, cout = shape
    x, dz, dzp, dzs, wt, w_d, prior = _grad_case(*shape)
    want = _dgrad_ref(*shape) + (prior.astype(np.float64) if acc else 0.0)
    L = g.L
    d = C.desc(n, h, w, cin, 0, cout, k, stride)
    gd = C.desc(n, h // stride, w // stride, dzs, 0, cin, k, 1)
    size_fn = {'wino': L.y3_conv_wino_workspace_bytes, 'wino44': L.y3_conv_wino44_workspace_bytes}.get(form, L.y3_conv_workspace_bytes)
    wsb = size_fn(ctypes.byref(gd)) if ws == 'exact' else 0
    if expect_streamk:
        assert wsb > 0 and L.y3_conv_schedule(ctypes.byref(gd), 0, 1) == C.STREAMK
    planes = {'split3': 3, 'split2': 2}.get(form, 0)
    wk = None
    if planes:
        wk = OUT('w_packed_d', (planes * k * k * cin * dzs,), BF16)
    elif form in ('wino', 'wino44'):
        wk = OUT('w_packed_d', ({'wino': 16, 'wino44': 36}[form] * cin * dzs,))
    specs = [IN('dz', dzp), IN('w_d', w_d), wk, IN('ones', np.ones(cin, np.float32)), IN('zeros', np.zeros(cin, np.float32)),
             INOUT('dx', prior) if acc else OUT('dx', (n, h, w, cin)), S('workspace', wsb)]

    def call(a):
        t = lambda name: P(a[name])
        tail = (t('ones'), t('zeros'), acc, t('dx'), t('workspace'), ctypes.c_size_t(wsb))
        if form == 'direct':
            g('y3_conv2d_dgrad', g.ctx, ctypes.byref(d), t('dz'), dzs, t('w_d'), *tail)
        elif planes:
            g('y3_pack_conv_weights_split_dgrad', g.ctx, t('w_d'), k, cin, dzs, planes, t('w_packed_d'))
            g('y3_conv2d_dgrad_split', g.ctx, ctypes.byref(d), planes, t('dz'), dzs, t('w_packed_d'), *tail)
        else:
            g('y3_pack_conv_weights_%s_dgrad' % form, g.ctx, t('w_d'), cin, dzs, t('w_packed_d'))
            g('y3_conv2d_dgrad_' + form, g.ctx, ctypes.byref(d), t('dz'), dzs, t('w_packed_d'), *tail)

    def verify(o):
        got = o['dx'].numpy()
        if form in ('direct', 'split3'):
            TS._check_elementwise(got, want, form)
        elif form == 'split2':
            TS._check_of_max(got, want, 5e-3, form)
        elif form == 'wino':
            assert np.isfinite(got).all() and rel_err(got, want) < 2e-4
        else:       # test_winograd_f4x4_data_gradient_matches_autograd: 2e-4 of the gradient's max (+ 1e-6 when accumulating)
            assert np.isfinite(got).all() and np.abs(got - want).max() <= 2e-4 * np.abs(_dgrad_ref(*shape)).max() + (1e-6 if acc else 0)
    return run_of(specs, call, ['dx'] + (['w_packed_d'] if wk is not None else []), verify)


# (n, h, w, k, stride, cin, cout): test_train_gpu's gradient shapes, the detection widths, the small stream-K case of
# conv_schedule_cases.DGRAD_S1
G_3X3 = (2, 20, 28, 3, 1, 64, 128)
G_1X1 = (2, 20, 28, 1, 1, 128, 64)
G_S2 = (3, 16, 24, 3, 2, 32, 64)
G_DET255 = (2, 13, 13, 1, 1, 256, 255)
G_DET18 = (2, 13, 13, 1, 1, 512, 18)
G_SK = (3, 37, 37, 3, 1, 128, 64)            # conv_schedule_cases.DGRAD_S1[0]: gradient conv -> 128 channels, 33 tiles, ragged M, odd map
G_W44 = (2, 13, 13, 3, 1, 64, 128)
for _acc in (0, 1):
    for _id, _shape in (('3x3', G_3X3), ('1x1', G_1X1), ('3x3s2', G_S2), ('det255', G_DET255), ('det18', G_DET18)):
        entry('conv_dgrad-%s-acc%d-null' % (_id, _acc), ('y3_conv2d_dgrad',), dgrad, _shape, 'direct', _acc)
    entry('conv_dgrad-streamk-acc%d-exact' % _acc, ('y3_conv2d_dgrad',), dgrad, G_SK, 'direct', _acc, ws='exact', expect_streamk=True)
    for _p in (3, 2):
        for _id, _shape in (('3x3', G_3X3), ('1x1', G_1X1), ('det255', G_DET255)):
            entry('conv_dgrad_split%d-%s-acc%d-null' % (_p, _id, _acc), ('y3_pack_conv_weights_split_dgrad', 'y3_conv2d_dgrad_split'),
                  dgrad, _shape, 'split%d' % _p, _acc)
        entry('conv_dgrad_split%d-streamk-acc%d-exact' % (_p, _acc), ('y3_pack_conv_weights_split_dgrad', 'y3_conv2d_dgrad_split'), dgrad,
              G_SK, 'split%d' % _p, _acc, ws='exact', expect_streamk=True)
    for _ws in ('null', 'exact'):
        entry('conv_dgrad_wino-3x3-acc%d-%s' % (_acc, _ws), ('y3_pack_conv_weights_wino_dgrad', 'y3_conv2d_dgrad_wino'), dgrad, G_3X3,
              'wino', _acc, ws=_ws)
        entry('conv_dgrad_wino44-2x13x13-acc%d-%s' % (_acc, _ws), ('y3_pack_conv_weights_wino44_dgrad', 'y3_conv2d_dgrad_wino44'),
              dgrad, G_W44, 'wino44', _acc, ws=_ws)


def dgrad_bn(g, case, acc):
    """y3_conv2d_dgrad_bn (conv_schedule_cases.DGRAD_BN) followed by y3_bn_train_bwd_partials on its partial rows: dx
    elementwise as above; d gamma, d beta and dz 2e-4 of max against fp64 autograd on the LeakyReLU branches the kernel takes
    (test_conv_schedules_gpu.test_fused_bn_backward_reduction (c))."""
    n, h, w, cin, cout, _, bm, sched = C.DGRAD_BN[case]
    dzs = _wider(cout)
    m = n * h * w
    L = g.L
    d = C.desc(n, h, w, cin, 0, cout, 1, 1)
    nblk = L.y3_conv_dgrad_bn_blocks(ctypes.byref(d))
    assert nblk == -(-m // bm)
    rng = np.random.RandomState(500 + case)
    z = (rng.standard_normal((m, cin)) * 2 + rng.standard_normal(cin)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.normal(0, 0.3, cin).astype(np.float32)
    dz = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    wt = (rng.standard_normal((1, 1, cin, cout)) * 0.1).astype(np.float32)
    prior = rng.standard_normal((m, cin)).astype(np.float32)
    z64 = z.astype(np.float64)
    mean, inv_std = z64.mean(0), 1.0 / np.sqrt(z64.var(0) + 1e-5)
    scale = gamma * inv_std
    vec = np.stack([mean, inv_std, scale, beta - mean * scale]).astype(np.float32)      # what y3_bn_train_stats hands over
    w_d = np.zeros((cin, dzs), np.float32)
    w_d[:, :cout] = wt.reshape(cin, cout)
    sb = L.y3_bn_bwd_scratch_bytes(cin)
    specs = [IN('dz', TS._pad_lanes(rng, dz, dzs)), IN('w_d', w_d), IN('ones', np.ones(cin, np.float32)),
             IN('zeros', np.zeros(cin, np.float32)), INOUT('dx', prior) if acc else OUT('dx', (m, cin)), IN('bn_z', z),
             IN('bn_vec', vec), OUT('partial', (nblk, 2, cin)), IN('gamma', gamma), OUT('dgamma', (cin,)), OUT('dbeta', (cin,)),
             OUT('dz_bn', (m, cin)), S('scratch', sb)]

    def call(a):
        t = lambda name: P(a[name])
        v = a['bn_vec']
        g('y3_conv2d_dgrad_bn', g.ctx, ctypes.byref(d), t('dz'), dzs, t('w_d'), t('ones'), t('zeros'), acc, t('dx'), t('bn_z'),
          t('bn_vec'), t('partial'))
        g('y3_bn_train_bwd_partials', g.ctx, t('bn_z'), t('dx'), t('gamma'), P(v[2]), P(v[3]), P(v[0]), P(v[1]), m, cin, t('partial'),
          nblk, t('dgamma'), t('dbeta'), t('dz_bn'), t('scratch'))

    def verify(o):
        got = o['dx'].numpy()
        TS._check_elementwise(got, TS.dgrad64(dz, wt, (m, cin), 1, 1) + (prior.astype(np.float64) if acc else 0.0), 'dx')
        mask = (z * vec[2] + vec[3]) > 0
        wg, wb, wz = TS._leaky_bn_autograd(z, gamma, beta, mask, got)
        for what, a, b in (('d gamma', o['dgamma'], wg), ('d beta', o['dbeta'], wb), ('dz', o['dz_bn'], wz)):
            TS._check_of_max(a.numpy().astype(np.float64), b, 2e-4, what)
    return run_of(specs, call, ['dx', 'partial', 'dgamma', 'dbeta', 'dz_bn'], verify)


for _case in (0, 1, 2, 4):        # the (3, 20, 28) cases: 128x32, 128x64 and 64x64 tiles, and the detection conv's 255 columns
    for _acc in (0, 1):
        entry('conv_dgrad_bn-case%d-acc%d' % (_case, _acc), ('y3_conv2d_dgrad_bn', 'y3_bn_train_bwd_partials'), dgrad_bn, _case, _acc)


def wgrad(g, shape, wino=False):
    """y3_conv_wgrad / y3_conv_wgrad_wino: scratch of exactly *_scratch_bytes (16-byte aligned), dw_hwio at a 4-byte boundary
    (the header: "dw_hwio itself: any 4-byte boundary"; the train step writes it at flat_grad + offset)."""
    n, h, w, k, stride, cin, cout = shape
    x, dz, dzp, dzs, wt, w_d, prior = _grad_case(*shape)
    want = _wgrad_ref(*shape)
    d = C.desc(n, h, w, cin, 0, cout, k, stride)
    if wino:
        assert g.L.y3_conv_wgrad_wino_eligible(ctypes.byref(d)) == 1
    sb = (g.L.y3_conv_wgrad_wino_scratch_bytes if wino else g.L.y3_conv_wgrad_scratch_bytes)(ctypes.byref(d))
    specs = [IN('x', x), IN('dz', dzp), OUT('dw_hwio', (k, k, cin, cout), align=4), S('scratch', sb)]

    def call(a):
        g('y3_conv_wgrad_wino' if wino else 'y3_conv_wgrad', g.ctx, ctypes.byref(d), P(a['x']), P(a['dz']), dzs, P(a['dw_hwio']),
          P(a['scratch']), ctypes.c_size_t(sb))
    return run_of(specs, call, ['dw_hwio'], lambda o: TS._check_of_max(o['dw_hwio'].numpy(), want, 2e-4, 'wgrad'))


W_3X3 = (3, 37, 37, 3, 1, 64, 128)           # conv_schedule_cases.WGRAD[3]: 43 splits x 3 K-steps, M % 32 = 11, Winograd-eligible
for _id, _shape in (('3x3', W_3X3), ('1x1_det18', (7, 26, 26, 1, 1, 512, 18)), ('1x1_det75', (3, 52, 50, 1, 1, 256, 75)),
                    ('1x1', (3, 61, 67, 1, 1, 128, 64)), ('3x3s2', G_S2), ('stem', (1, 9, 130, 3, 1, 3, 32)), ('det255', G_DET255)):
    entry('conv_wgrad-' + _id, ('y3_conv_wgrad',), wgrad, _shape)
for _id, _shape in (('3x37x37', W_3X3), ('1x13x13', (1, 13, 13, 3, 1, 128, 64)), ('3x7x5', (3, 7, 5, 3, 1, 64, 64))):
    entry('conv_wgrad_wino-' + _id, ('y3_conv_wgrad_wino',), wgrad, _shape, wino=True)


# ---- the same entries cut into image ranges (one buffer resource per range) ---------------------------------------------
def cut_into_ranges(g, builder, fwd_desc, *args, **kw):
    """`builder`'s case with the launch cut into ranges of 2, 2 and 1 images by the test hook y3_debug_conv_range_limit, as
    tests/test_conv_ranges_gpu.py does (n = 5, a limit of two images plus one element; restored in a `finally`).  The size
    functions are asked under the same limit: a cut launch has its own scratch and partial-row counts."""
    d = C.desc(*fwd_desc)
    dzs = 0 if builder is conv_fwd else (d.cout if d.cin == 3 else _wider(d.cout))
    limit = TR.two_image_limit(d, dzs)
    TR.assert_cut(g.L, d, dzs, limit)
    with TR.lowered(limit):
        run = builder(g, *args, **kw)

    def call(a):
        with TR.lowered(limit):
            run.call(a)
    return run._replace(call=call)


def _fwd_desc(shape):       # a conv_fwd shape or a gradient shape -> (n, h, w, cin, c_up, cout, k, stride)
    if len(shape) == 10:
        n, h, w, k, stride, cin, cout, act, resid, c_up = shape
    else:
        (n, h, w, k, stride, cin, cout), c_up = shape, 0
    return (n, h, w, cin, c_up, cout, k, stride)


CUT_FWD = [('3x3s1_res', (5, 10, 14, 3, 1, 32, 64, 1, True, 0), 'direct'),
           ('3x3s2_odd_rows', (5, 26, 30, 3, 2, 64, 128, 1, False, 0), 'direct'),   # 195 rows per image: ranges end inside a tile
           ('head255', (5, 13, 13, 1, 1, 256, 255, 0, False, 0), 'direct'),
           ('stem_odd', (5, 33, 37, 3, 1, 3, 32, 1, False, 0), 'direct'),           # 1221 pixels per image
           ('3x3s1_res', (5, 10, 14, 3, 1, 32, 64, 1, True, 0), 'split3'),
           ('head255', (5, 13, 13, 1, 1, 256, 255, 0, False, 0), 'split2')]
for _id, _shape, _form in CUT_FWD:
    _covers = ('y3_conv2d_fwd',) if _shape[5] == 3 else (('y3_pack_conv_weights', 'y3_conv2d_fwd') if _form == 'direct' else
                                                         ('y3_pack_conv_weights_split', 'y3_conv2d_fwd_split'))
    entry('conv_fwd%s-%s-cut' % ('' if _form == 'direct' else '_' + _form, _id), _covers, cut_into_ranges, conv_fwd, _fwd_desc(_shape),
          _shape, form=_form)
_CUT_STATS = (5, 13, 13, 1, 1, 128, 64, 0, False, 0)
entry('conv_fwd_stats-1x1-cut', ('y3_pack_conv_weights', 'y3_conv2d_fwd_stats', 'y3_bn_train_stats_partials'), cut_into_ranges, conv_fwd,
      _fwd_desc(_CUT_STATS), _CUT_STATS, stats=True)
CUT_3X3, CUT_S2, CUT_DET, CUT_STEM = (5, 13, 13, 3, 1, 64, 128), (5, 16, 24, 3, 2, 32, 64), (5, 13, 13, 1, 1, 256, 255), (5, 33, 37, 3, 1, 3, 32)
for _acc in (0, 1):
    for _id, _shape in (('3x3', CUT_3X3), ('3x3s2', CUT_S2), ('det255', CUT_DET)):
        entry('conv_dgrad-%s-acc%d-cut' % (_id, _acc), ('y3_conv2d_dgrad',), cut_into_ranges, dgrad, _fwd_desc(_shape), _shape, 'direct', _acc)
    entry('conv_dgrad_split3-3x3-acc%d-cut' % _acc, ('y3_pack_conv_weights_split_dgrad', 'y3_conv2d_dgrad_split'), cut_into_ranges, dgrad,
          _fwd_desc(CUT_3X3), CUT_3X3, 'split3', _acc)
for _id, _shape in (('3x3', CUT_3X3), ('3x3s2', CUT_S2), ('det255', CUT_DET), ('stem_odd', CUT_STEM)):
    entry('conv_wgrad-%s-cut' % _id, ('y3_conv_wgrad',), cut_into_ranges, wgrad, _fwd_desc(_shape), _shape)


# ============================================================================================================================
# Batch norm and column reductions.  Reference: fp64 autograd of leaky(BN_train(z)) + residual; tolerances of
# test_train_gpu.test_bn_train_forward_backward (mean 1e-5, y 2e-5, moving rtol 1e-5 / atol 1e-6, gradients 2e-4 of max) and
# check_bn_statistics above.
# ============================================================================================================================
BN_SHAPES = [(3, 256), (600, 1028), (338, 64), (43527, 12)]


@functools.lru_cache(maxsize=None)
def _bn_case(rows, c, bf16_z=False):
    rng = np.random.RandomState(rows + c)
    zt = torch.tensor(rng.standard_normal((rows, c)) * 2 + rng.standard_normal(c), dtype=torch.float32)
    if bf16_z:
        zt = zt.to(BF16)
    z = zt.to(torch.float64).requires_grad_(True)
    gamma = torch.tensor(rng.uniform(0.5, 1.5, c), dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(rng.normal(0, 0.3, c), dtype=torch.float64, requires_grad=True)
    resid = rng.standard_normal((rows, c)).astype(np.float32)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    u = (z - mean) * gamma / torch.sqrt(var + 1e-5) + beta
    y = torch.where(u > 0, u, 0.1 * u) + torch.tensor(resid, dtype=torch.float64)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    f = lambda t: t.detach().numpy()
    return dict(zt=zt, gamma=f(gamma).astype(np.float32), beta=f(beta).astype(np.float32), resid=resid, dy=dy, y=f(y), mean=f(mean),
                var=f(var), dgamma=f(gamma.grad), dbeta=f(beta.grad), dz=f(z.grad))


def _bn_specs(cs, c, with_moving=True):
    return [IN('gamma', cs['gamma']), IN('beta', cs['beta']), OUT('mean', (c,)), OUT('inv_std', (c,)), OUT('scale', (c,)),
            OUT('shift', (c,))] + ([INOUT('moving_mean', np.full(c, 0.25, np.float32)),
                                    INOUT('moving_var', np.full(c, 2.0, np.float32))] if with_moving else [])


def _verify_bn_fwd(cs, o, rows):
    assert rel_err(o['mean'].numpy(), cs['mean']) < 1e-5
    np.testing.assert_allclose(o['moving_mean'].numpy(), 0.25 * 0.9 + cs['mean'] * 0.1, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o['moving_var'].numpy(), 2.0 * 0.9 + cs['var'] * rows / (rows - 1.0) * 0.1, rtol=1e-5, atol=1e-6)
    assert rel_err(o['y'].numpy(), cs['y']) < 2e-5


def _verify_bn_bwd(cs, o):
    assert rel_err(o['dgamma'].numpy(), cs['dgamma']) < 2e-4
    assert rel_err(o['dbeta'].numpy(), cs['dbeta']) < 2e-4
    assert rel_err(npf(o['dz']), cs['dz']) < 2e-4


def bn_train(g, rows, c):
    """y3_bn_train_stats (scratch: exactly y3_reduce_scratch_bytes(c)) -> y3_bn_apply_fwd -> y3_bn_train_bwd (scratch: exactly
    y3_bn_bwd_scratch_bytes(c))."""
    cs = _bn_case(rows, c)
    rb, bb = g.L.y3_reduce_scratch_bytes(c), g.L.y3_bn_bwd_scratch_bytes(c)
    specs = [IN('z', cs['zt'])] + _bn_specs(cs, c) + [IN('residual', cs['resid']), OUT('y', (rows, c)), IN('dy', cs['dy']),
                                                        OUT('dgamma', (c,)), OUT('dbeta', (c,)), OUT('dz', (rows, c)),
                                                        S('reduce_scratch', rb), S('bwd_scratch', bb)]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_bn_train_stats', g.ctx, t('z'), rows, c, t('gamma'), t('beta'), cf(1e-5), cf(0.9), t('mean'), t('inv_std'), t('scale'),
          t('shift'), t('moving_mean'), t('moving_var'), t('reduce_scratch'))
        g('y3_bn_apply_fwd', g.ctx, t('z'), t('scale'), t('shift'), t('residual'), rows, c, 1, t('y'))
        g('y3_bn_train_bwd', g.ctx, t('z'), t('dy'), t('gamma'), t('scale'), t('shift'), t('mean'), t('inv_std'), rows, c, t('dgamma'),
          t('dbeta'), t('dz'), t('bwd_scratch'))

    def verify(o):
        _verify_bn_fwd(cs, o, rows)
        _verify_bn_bwd(cs, o)
    return run_of(specs, call, ['mean', 'inv_std', 'scale', 'shift', 'moving_mean', 'moving_var', 'y', 'dgamma', 'dbeta', 'dz'], verify)


for _rows, _c in BN_SHAPES:
    entry('bn_train-%dx%d' % (_rows, _c), ('y3_bn_train_stats', 'y3_bn_apply_fwd', 'y3_bn_train_bwd'), bn_train, _rows, _c)


def bn_sync(g, rows, c, bf16_z):
    """The four halves on one shard with the buffer left alone (sums: double[2c + 1] at an 8-byte boundary), against fp64 batch
    norm at the tolerances of test_sync_bn_kernels_gpu.py (those of bn_train; a bf16 dz adds its one rounding)."""
    cs = _bn_case(rows, c, bf16_z)
    bb = g.L.y3_bn_bwd_scratch_bytes(c)
    b16 = 1 if bf16_z else 0
    specs = [IN('z', cs['zt'])] + _bn_specs(cs, c) + [IN('residual', cs['resid']), IN('z_f32', cs['zt'].float()), OUT('y', (rows, c)),
                                                        IN('dy', cs['dy']), OUT('dgamma', (c,)), OUT('dbeta', (c,)),
                                                        OUT('dz', (rows, c), BF16 if bf16_z else F32),
                                                        OUT('sums', (2 * c + 1,), F64, align=8), S('scratch', bb)]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_bn_sync_stats_sums', g.ctx, t('z'), b16, None, 0, rows, c, t('sums'), t('scratch'))
        g('y3_bn_sync_stats_finish', g.ctx, t('sums'), c, t('gamma'), t('beta'), cf(1e-5), cf(0.9), t('mean'), t('inv_std'), t('scale'),
          t('shift'), t('moving_mean'), t('moving_var'))
        g('y3_bn_apply_fwd', g.ctx, t('z_f32'), t('scale'), t('shift'), t('residual'), rows, c, 1, t('y'))
        g('y3_bn_sync_bwd_sums', g.ctx, t('z'), b16, t('dy'), t('scale'), t('shift'), t('mean'), t('inv_std'), rows, c, None, 0,
          t('dgamma'), t('dbeta'), t('sums'), t('scratch'))
        g('y3_bn_sync_bwd_finish', g.ctx, t('z'), b16, t('dy'), t('gamma'), t('scale'), t('shift'), t('mean'), t('inv_std'), rows, c,
          t('sums'), t('dz'), t('scratch'))

    def verify(o):
        _verify_bn_fwd(cs, o, rows)
        assert float(o['sums'][2 * c]) == rows
        if bf16_z:
            want, dz = cs['dz'], npf(o['dz'])
            e = 2e-4 * np.abs(want).max()
            assert (np.abs(dz - want) <= e + 2.0 ** -8 * (np.abs(want) + e)).all()
            assert rel_err(o['dgamma'].numpy(), cs['dgamma']) < 2e-4 and rel_err(o['dbeta'].numpy(), cs['dbeta']) < 2e-4
        else:
            _verify_bn_bwd(cs, o)
    return run_of(specs, call, ['mean', 'inv_std', 'scale', 'shift', 'moving_mean', 'moving_var', 'y', 'dgamma', 'dbeta', 'dz', 'sums'],
                  verify)


_SYNC = ('y3_bn_sync_stats_sums', 'y3_bn_sync_stats_finish', 'y3_bn_apply_fwd', 'y3_bn_sync_bwd_sums', 'y3_bn_sync_bwd_finish')
for _rows, _c in BN_SHAPES[:3]:
    entry('bn_sync-%dx%d' % (_rows, _c), _SYNC, bn_sync, _rows, _c, False)
entry('bn_sync-256x64-bf16', _SYNC, bn_sync, 256, 64, True)


def bn_sync_from_partials(g, rows, c, nblk):
    """y3_bn_sync_stats_sums on the partial rows of a conv epilogue (z and scratch NULL), then the finish half: the statistics
    of the z whose column sums the partials are."""
    rng = np.random.RandomState(c)
    z = (rng.standard_normal((rows, c)) * 2 + rng.standard_normal(c)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.3, c).astype(np.float32)
    zb = np.zeros((nblk * -(-rows // nblk), c), np.float64)
    zb[:rows] = z
    zb = zb.reshape(nblk, -1, c)
    part = np.stack([zb.sum(1), (zb * zb).sum(1)], 1).astype(np.float32)
    specs = [IN('partial', part)] + _bn_specs(dict(gamma=gamma, beta=beta), c) + [OUT('sums', (2 * c + 1,), F64, align=8)]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_bn_sync_stats_sums', g.ctx, None, 0, t('partial'), nblk, rows, c, t('sums'), None)
        g('y3_bn_sync_stats_finish', g.ctx, t('sums'), c, t('gamma'), t('beta'), cf(1e-5), cf(0.9), t('mean'), t('inv_std'), t('scale'),
          t('shift'), t('moving_mean'), t('moving_var'))

    def verify(o):
        bn = np.stack([o[k].numpy() for k in ('mean', 'inv_std', 'scale', 'shift')])
        check_bn_statistics(z, gamma, beta, bn, o['moving_mean'].numpy(), o['moving_var'].numpy())
    return run_of(specs, call, ['mean', 'inv_std', 'scale', 'shift', 'moving_mean', 'moving_var', 'sums'], verify)


entry('bn_sync_from_partials-338x64', ('y3_bn_sync_stats_sums', 'y3_bn_sync_stats_finish'), bn_sync_from_partials, 338, 64, 6)


# ============================================================================================================================
# Routing.  The parametrisations, references and gates of test_routing_gpu.py (bit for bit; y3_bias_grad within the bound of
# its fp32 partial sums).
# ============================================================================================================================
def upsample2x_bwd(g, n, h, w, c, gc, off, acc):
    rng = np.random.RandomState(n * 1000 + h * 10 + c + acc)
    gr = rng.standard_normal((n, 2 * h, 2 * w, gc)).astype(np.float32)
    old = rng.standard_normal((n, h, w, c)).astype(np.float32)
    gs = gr[..., off:off + c]
    want = ((gs[:, 0::2, 0::2] + gs[:, 0::2, 1::2]) + gs[:, 1::2, 0::2]) + gs[:, 1::2, 1::2]
    want = old + want if acc else want
    specs = [IN('g', gr), INOUT('dx', old) if acc else OUT('dx', (n, h, w, c))]

    def call(a):
        g('y3_upsample2x_bwd', g.ctx, ctypes.c_void_p(a['g'].data_ptr() + 4 * off), gc, n, h, w, c, acc, P(a['dx']))
    return run_of(specs, call, ['dx'], lambda o: np.testing.assert_array_equal(o['dx'].numpy(), want))


for _acc in (0, 1):
    for _a in [(2, 3, 5, 8, 8, 0), (1, 13, 13, 128, 384, 128), (3, 4, 4, 4, 12, 4), (2, 52, 52, 256, 256, 0), (1, 105, 105, 384, 384, 0)]:
        entry('upsample2x_bwd-%dx%dx%dx%d-g%d+%d-acc%d' % (_a + (_acc,)), ('y3_upsample2x_bwd',), upsample2x_bwd, *(_a + (_acc,)))


def slice_accumulate(g, rows, sc, off, c, acc):
    rng = np.random.RandomState(rows + sc + off + c + acc)
    src = rng.standard_normal((rows, sc)).astype(np.float32)
    old = rng.standard_normal((rows, c)).astype(np.float32)
    want = old + src[:, off:off + c] if acc else src[:, off:off + c]
    specs = [IN('src', src), INOUT('dst', old) if acc else OUT('dst', (rows, c))]

    def call(a):
        g('y3_slice_accumulate', g.ctx, P(a['src']), sc, off, rows, c, acc, P(a['dst']))
    return run_of(specs, call, ['dst'], lambda o: np.testing.assert_array_equal(o['dst'].numpy(), want))


for _acc in (0, 1):
    for _a in [(7, 12, 4, 8), (338, 768, 256, 512), (5, 8, 0, 8), (1, 4, 0, 4), (3, 16, 12, 4)]:
        entry('slice_accumulate-%dx%d+%d:%d-acc%d' % (_a + (_acc,)), ('y3_slice_accumulate',), slice_accumulate, *(_a + (_acc,)))


def pad_channels(g, rows, cs, cd):
    src = np.random.RandomState(rows + cs + cd).standard_normal((rows, cs)).astype(np.float32)
    want = np.zeros((rows, cd), np.float32)
    want[:, :cs] = src

    def call(a):
        g('y3_pad_channels', g.ctx, P(a['src']), cs, rows, cd, P(a['dst']))
    return run_of([IN('src', src), OUT('dst', (rows, cd))], call, ['dst'], lambda o: np.testing.assert_array_equal(o['dst'].numpy(), want))


for _a in [(169, 255, 256), (10, 18, 32), (4, 75, 96), (3, 8, 8)]:
    entry('pad_channels-%dx%d->%d' % _a, ('y3_pad_channels',), pad_channels, *_a)


def bias_grad(g, rows, c):
    """scratch: exactly the header's 1024 * c floats"""
    dy = np.random.RandomState(rows + c).standard_normal((rows, c)).astype(np.float32)

    def call(a):
        g('y3_bias_grad', g.ctx, P(a['dy']), rows, c, P(a['dbias']), P(a['scratch']))

    def verify(o):
        d64 = dy.astype(np.float64)
        nb = min(rows, 512)
        bound = (-(-rows // nb) + 1) * U * np.abs(d64).sum(0)
        assert np.all(np.abs(o['dbias'].numpy().astype(np.float64) - d64.sum(0)) <= bound)
    return run_of([IN('dy', dy), OUT('dbias', (c,)), S('scratch', 1024 * c * 4)], call, ['dbias'], verify)


for _a in [(338, 255), (1, 18), (600, 75), (5000, 300)]:
    entry('bias_grad-%dx%d' % _a, ('y3_bias_grad',), bias_grad, *_a)


# ============================================================================================================================
# Loss and optimizer.
# ============================================================================================================================
def loss_layer(g, case, smooth, focal):
    """test_loss_gpu.py's smallest off-square case: each term within 1e-4 |ref| + 1e-6, the gradient 2e-4 of max; the rows of
    grad are padded to a multiple of 32 and the pad lanes must stay as they were (here: the poison)."""
    n, gh, gw, H, W, Cn, scale, seed = TL.CASES[case]
    fm, y = TL.inputs(case)
    want4, wantg = TL.reference(case, smooth, focal)
    lanes, stride = TL._strides(case, False)
    sb = g.L.y3_loss_scratch_bytes(n, gh, gw)
    ancp = host_f32(TL._anchors(scale))
    specs = [IN('feature_map', fm), IN('y_true', y), OUT('loss4', (4,)), OUT('grad', (n, gh, gw, stride)), S('scratch', sb)]

    def call(a):
        g('y3_loss_layer', g.ctx, P(a['feature_map']), P(a['y_true']), n, gh, gw, Cn, H, W, ancp, int(smooth), int(focal), 0,
          P(a['loss4']), P(a['grad']), stride, P(a['scratch']), ctypes.c_size_t(sb))

    def view(o, byte):
        pad = o['grad'][..., lanes:].contiguous().view(U8)
        assert bool((pad == byte).all()), 'a pad lane of grad was written'
        return dict(loss4=o['loss4'], grad=o['grad'][..., :lanes].contiguous())

    def verify(o):
        for name, a, b in zip(('xy', 'wh', 'conf', 'class'), o['loss4'].tolist(), want4):
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (name, a, b)
        gnp = o['grad'].numpy()
        assert np.isfinite(gnp).all() and TL.rel_err(gnp, wantg) < 2e-4
    return run_of(specs, call, ['loss4', 'grad'], verify, view)


for _s, _f in ((False, False), (True, True)):
    entry('loss_layer-1x2_c1-smooth%d-focal%d' % (_s, _f), ('y3_loss_layer',), loss_layer, '1x2_c1', _s, _f)

OPT_SIZES = (1, 3, 4, 4099)
OPT_NORM = (300.0, 30.0, 300.0, 30.0)        # of grad_scale * g: above / below the clip norm of 100
OPT_WD = (0.0, 5e-4, 5e-4, 0.0)


@functools.lru_cache(maxsize=None)
def _opt_case(kind, sizes):
    """test_optimizer_gpu._inputs' recipe on this file's lengths, and its fp64 expectation (_expected: oracle/train_ref.py)."""
    r = np.random.RandomState(2000 + TO.KINDS.index(kind))
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    out = []
    for n in sizes:
        i = OPT_SIZES.index(n)
        el = min(OPT_NORM[i], TO.HP['clip']) / np.sqrt(n)
        w, gr = r.standard_normal(n), r.standard_normal(n) * OPT_NORM[i] / (TO.HP['gs'] * np.sqrt(n))
        if n == 1:
            gr = np.array([OPT_NORM[i] / TO.HP['gs']])
        s0 = s1 = None
        if kind == 'momentum':
            s0 = r.standard_normal(n) * 2 * el
        elif kind == 'adam':
            s0, s1 = r.standard_normal(n) * 0.5 * el, (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2
        elif kind == 'rmsprop':
            s0, s1 = (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2, r.standard_normal(n) * 0.01
        out.append(dict(w=f(w), g=f(gr), s0=f(s0), s1=f(s1), wd=OPT_WD[i]))
    return out, TO._expected(kind, out)


def _opt_verify(o, want, tensors):
    """test_optimizer_gpu.TOL: 2e-6 of each output tensor's max |expected|"""
    for i, e in enumerate(want):
        for key in ('w', 'g', 's0', 's1'):
            if e[key] is not None:
                got = o['%s%d' % (key, i)].numpy().astype(np.float64)
                assert np.abs(got - e[key]).max() <= TO.TOL * np.abs(e[key]).max(), (key, i)


def _opt_specs(inputs):
    """tensors with n % 4 != 0 at a 4-byte boundary, as the header allows; the others at 16"""
    specs = []
    for i, t in enumerate(inputs):
        al = 16 if t['w'].size % 4 == 0 else 4
        specs += [INOUT('%s%d' % (k, i), t[k], align=al) for k in ('w', 'g', 's0', 's1') if t[k] is not None]
    return specs


def _opt_hp(kind):
    hp = TO.HP
    lr = TO._lr_t(hp['lr'], hp['beta1'], hp['beta2'], hp['step']) if kind == 'adam' else hp['lr']
    return (cf(hp['gs']), cf(hp['clip']), cf(lr), cf(hp['momentum']), cf(hp['beta1'] if kind == 'adam' else hp['decay']),
            cf(hp['beta2']), cf(TO.EPS[kind]))


def clip_update(g, kind, n):
    inputs, want = _opt_case(kind, (n,))
    sb = g.L.y3_optimizer_scratch_bytes()
    specs = _opt_specs(inputs) + [S('scratch', sb)]
    names = [s.name for s in specs]

    def call(a):
        t = lambda k: P(a[k]) if k in names else None
        g('y3_clip_update', g.ctx, TO.KINDS.index(kind), t('w0'), t('g0'), t('s00'), t('s10'), n, cf(inputs[0]['wd']),
          *(_opt_hp(kind) + (t('scratch'),)))
    return run_of(specs, call, names[:-1], lambda o: _opt_verify(o, want, inputs))


def clip_update_multi(g, kind, sizes):
    inputs, want = _opt_case(kind, sizes)
    arr0 = (g._lib.ParamDesc * len(inputs))()
    for i, t in enumerate(inputs):
        arr0[i] = g._lib.ParamDesc(None, None, None, None, t['w'].size, t['wd'], 0)
    sb = g.L.y3_clip_update_multi_scratch_bytes(arr0, len(inputs))      # (it reads the lengths only)
    specs = _opt_specs(inputs) + [S('scratch', sb)]
    names = [s.name for s in specs]

    def call(a):
        dp = lambda k: a[k].data_ptr() if k in names else None
        arr = (g._lib.ParamDesc * len(inputs))()
        for i, t in enumerate(inputs):
            arr[i] = g._lib.ParamDesc(dp('w%d' % i), dp('g%d' % i), dp('s0%d' % i), dp('s1%d' % i), t['w'].size, t['wd'], 0)
        assert g.L.y3_clip_update_multi_scratch_bytes(arr, len(inputs)) == sb
        g('y3_clip_update_multi', g.ctx, TO.KINDS.index(kind), arr, len(inputs), *(_opt_hp(kind) + (P(a['scratch']), ctypes.c_size_t(sb))))
    return run_of(specs, call, names[:-1], lambda o: _opt_verify(o, want, inputs))


for _kind in TO.KINDS:
    for _n in OPT_SIZES:
        entry('clip_update-%s-n%d' % (_kind, _n), ('y3_clip_update',), clip_update, _kind, _n)
    entry('clip_update_multi-%s' % _kind, ('y3_clip_update_multi',), clip_update_multi, _kind, (4099, 1, 4, 3, 3, 4, 1, 4099))


# ============================================================================================================================
# bf16 training kernels.  References and gates: test_train_bf16_kernels_gpu.py (fp64 on the same bf16-exact operands; bf16
# outputs within one rounding (2.05 units of within_one_rounding); partial sums 4e-7; dgrad 1.2e-6; wgrad 5e-7; d gamma, d beta
# 3e-7 of max).
# ============================================================================================================================
def train_fwd_bf16(g, n, h, w, k, stride, cin, cout):
    rng = np.random.RandomState(cin + cout + k)
    x = TK.bf16_exact(rng, (n, h, w, cin))
    wt = torch.tensor(rng.standard_normal((k, k, cin, cout)) * 0.1, dtype=torch.float32)
    ref = TK.conv_ref(x.double(), wt.to(BF16).double(), k, stride)
    d = C.desc(n, h, w, cin, 0, cout, k, stride)
    ho, wo = h // stride, w // stride
    nb = g.L.y3_conv_train_stats_blocks_bf16(ctypes.byref(d))
    assert nb == (n * ho * wo + 127) // 128
    specs = [IN('x', x), IN('w_hwio', wt), OUT('w_packed', (k * k * cin * cout,), BF16), OUT('z', (n, ho, wo, cout), BF16),
             OUT('stats', (nb, 2, cout))]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_pack_conv_weights_bf16_train', g.ctx, t('w_hwio'), k, cin, cout, 0, t('w_packed'))
        g('y3_conv2d_train_fwd_bf16', g.ctx, ctypes.byref(d), t('x'), t('w_packed'), t('z'), t('stats'))

    def verify(o):
        zc, stc = o['z'].double(), o['stats'].double()
        assert TK.within_one_rounding(zc, ref) <= 2.05
        zr = zc.reshape(-1, cout)
        s = stc.sum(0)
        assert TK.rel_err(s[0], zr.sum(0)) < 4e-7 and TK.rel_err(s[1], (zr ** 2).sum(0)) < 4e-7
        zb = torch.zeros((nb * 128, cout), dtype=torch.float64)
        zb[:zr.shape[0]] = zr
        zb = zb.reshape(nb, 128, cout)
        want_b = torch.stack([zb.sum(1), (zb ** 2).sum(1)], 1)
        assert float(((stc - want_b).abs().amax(2) / want_b.abs().amax(2).clamp_min(1e-12)).max()) < 4e-7
    return run_of(specs, call, ['z', 'stats', 'w_packed'], verify)


for _a in [(1, 6, 10, 1, 1, 32, 64), (1, 10, 14, 3, 1, 32, 20), (2, 13, 13, 1, 1, 128, 36), (2, 13, 13, 3, 1, 64, 192),
           (2, 26, 26, 3, 2, 64, 128), (2, 20, 28, 1, 1, 64, 32)]:
    entry('train_fwd_bf16-%dx%dx%d-k%ds%d-%d->%d' % _a, ('y3_pack_conv_weights_bf16_train', 'y3_conv2d_train_fwd_bf16'), train_fwd_bf16, *_a)


def _junk_lanes(rng, dz, dzs):
    out = TK.bf16_exact(rng, tuple(dz.shape[:3]) + (dzs,))
    out[..., :dz.shape[3]] = dz
    return out


def dgrad_bf16(g, n, h, w, k, stride, cin, cout, acc):
    dzs = _wider(cout)
    dz, wt, grad, prior = TK._dgrad_case(n, h, w, k, stride, cin, cout)
    want = grad + (prior.double() if acc else 0)
    d = C.desc(n, h, w, cin, 0, cout, k, stride)
    specs = [IN('dz', _junk_lanes(np.random.RandomState(cout), dz, dzs)), IN('w_hwio', wt), OUT('w_packed_d', (k * k * dzs * cin,), BF16),
             INOUT('dx', prior) if acc else OUT('dx', (n, h, w, cin))]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_pack_conv_weights_bf16_train', g.ctx, t('w_hwio'), k, cin, cout, dzs, t('w_packed_d'))
        g('y3_conv2d_dgrad_bf16', g.ctx, ctypes.byref(d), t('dz'), dzs, t('w_packed_d'), acc, t('dx'))
    return run_of(specs, call, ['dx', 'w_packed_d'],
                  lambda o: TK.rel_err(o['dx'], want) < TK.DGRAD_GATE.get((n, h, w, k, stride, cin, cout), 1.2e-6) or pytest.fail('dgrad'))


for _acc in (0, 1):
    for _a in [(1, 10, 26, 3, 2, 32, 96), (2, 13, 13, 3, 1, 192, 64), (2, 20, 28, 1, 1, 64, 32), (2, 13, 13, 1, 1, 256, 255),
               (2, 26, 26, 3, 2, 64, 128)]:
        entry('dgrad_bf16-%dx%dx%d-k%ds%d-%d->%d-acc%d' % (_a + (_acc,)), ('y3_pack_conv_weights_bf16_train', 'y3_conv2d_dgrad_bf16'),
              dgrad_bf16, *(_a + (_acc,)))


def wgrad_bf16(g, n, h, w, k, stride, cin, cout):
    """scratch: exactly y3_conv_wgrad_bf16_scratch_bytes (0: NULL); dw_hwio at a 4-byte boundary, as the train step places it"""
    rng = np.random.RandomState(3 * cin + cout + k)
    dzs = _wider(cout)
    ho, wo = h // stride, w // stride
    x, dz = TK.bf16_exact(rng, (n, h, w, cin)), TK.bf16_exact(rng, (n, ho, wo, cout))
    wv = torch.zeros((k, k, cin, cout), dtype=torch.float64, requires_grad=True)
    TK.conv_ref(x.double(), wv, k, stride).backward(dz.double())
    d = C.desc(n, h, w, cin, 0, cout, k, stride)
    sb = g.L.y3_conv_wgrad_bf16_scratch_bytes(ctypes.byref(d))
    splits = TK.WGRAD_SPLITS.get((n, h, w, k, stride, cin, cout))
    if splits is not None:
        assert sb == (splits * k * k * cin * cout * 4 if splits > 1 else 0)
    specs = [IN('x', x), IN('dz', _junk_lanes(rng, dz, dzs)), OUT('dw_hwio', (k, k, cin, cout), align=4), S('scratch', sb)]

    def call(a):
        g('y3_conv_wgrad_bf16', g.ctx, ctypes.byref(d), P(a['x']), P(a['dz']), dzs, P(a['dw_hwio']), P(a['scratch']), ctypes.c_size_t(sb))
    return run_of(specs, call, ['dw_hwio'], lambda o: TK.rel_err(o['dw_hwio'], wv.grad) < 5e-7 or pytest.fail('wgrad'))


for _a in [(2, 20, 28, 1, 1, 64, 32), (1, 6, 10, 1, 1, 32, 64), (2, 13, 13, 3, 1, 64, 192), (2, 25, 41, 1, 1, 128, 64),
           (2, 13, 13, 1, 1, 512, 18), (2, 26, 26, 3, 2, 64, 128)]:
    entry('wgrad_bf16-%dx%dx%d-k%ds%d-%d->%d' % _a, ('y3_conv_wgrad_bf16',), wgrad_bf16, *_a)


def bn_bf16(g, rows, c):
    """y3_bn_apply_fwd_bf16 and y3_bn_train_bwd_bf16 on bf16 z, with the layer's vectors from fp64 statistics of the same z."""
    rng = np.random.RandomState(rows + c)
    zb = torch.tensor(rng.standard_normal((rows, c)) * 2 + rng.standard_normal(c), dtype=torch.float32).to(BF16)
    z = zb.double().requires_grad_(True)
    gamma = torch.tensor(rng.uniform(0.5, 1.5, c), dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(rng.normal(0, 0.3, c), dtype=torch.float64, requires_grad=True)
    resid = TK.bf16_exact(rng, (rows, c))
    mean, var = z.mean(0), z.var(0, unbiased=False)
    inv_std = 1.0 / torch.sqrt(var + 1e-5)
    u = (z - mean) * gamma * inv_std + beta
    y = torch.where(u > 0, u, 0.1 * u)
    dy = torch.tensor(rng.standard_normal((rows, c)), dtype=torch.float32)
    y.backward(dy.double())
    scale = (gamma * inv_std).detach()
    f = lambda t: t.detach().float()
    sb = g.L.y3_bn_bwd_scratch_bytes(c)
    specs = [IN('z', zb), IN('scale', f(scale)), IN('shift', f(beta.detach() - mean.detach() * scale)), IN('mean', f(mean)),
             IN('inv_std', f(inv_std)), IN('gamma', f(gamma)), IN('residual', resid), OUT('y', (rows, c), BF16), IN('dy', dy),
             OUT('dgamma', (c,)), OUT('dbeta', (c,)), OUT('dz', (rows, c), BF16), S('scratch', sb)]

    def call(a):
        t = lambda name: P(a[name])
        g('y3_bn_apply_fwd_bf16', g.ctx, t('z'), 0, t('scale'), t('shift'), t('residual'), rows, c, t('y'))
        g('y3_bn_train_bwd_bf16', g.ctx, t('z'), t('dy'), t('gamma'), t('scale'), t('shift'), t('mean'), t('inv_std'), rows, c,
          t('dgamma'), t('dbeta'), t('dz'), t('scratch'))

    def verify(o):
        assert TK.within_one_rounding(o['y'].double(), y.detach() + resid.double()) <= 2.05
        assert TK.rel_err(o['dgamma'], gamma.grad) < 3e-7 and TK.rel_err(o['dbeta'], beta.grad) < 3e-7
        assert TK.within_one_rounding(o['dz'].double(), z.grad) <= 2.05
    return run_of(specs, call, ['y', 'dgamma', 'dbeta', 'dz'], verify)


for _rows, _c in BN_SHAPES:
    entry('bn_bf16-%dx%d' % (_rows, _c), ('y3_bn_apply_fwd_bf16', 'y3_bn_train_bwd_bf16'), bn_bf16, _rows, _c)


def upsample_concat_bf16(g, n, h, w, cu, cx):
    gen = torch.Generator().manual_seed(n + h + w)
    bits = lambda shape: (torch.randint(0, 2 ** 16, shape, generator=gen, dtype=torch.int32) - 2 ** 15).to(torch.int16)
    up, xr = bits((n, h // 2, w // 2, cu)), bits((n, h, w, cx))
    want = torch.cat([up.repeat_interleave(2, 1).repeat_interleave(2, 2), xr], -1)
    specs = [IN('up', up.view(BF16)), IN('x', xr.view(BF16)), OUT('out', (n, h, w, cu + cx), BF16)]

    def call(a):
        g('y3_upsample_concat_bf16', g.ctx, P(a['up']), cu, P(a['x']), cx, n, h, w, P(a['out']))
    return run_of(specs, call, ['out'], lambda o: torch.equal(o['out'].view(torch.int16), want) or pytest.fail('not an exact copy'))


entry('upsample_concat_bf16-3x6x10-12+20', ('y3_upsample_concat_bf16',), upsample_concat_bf16, 3, 6, 10, 12, 20)


def f32_to_bf16(g, count):
    v = torch.tensor(np.random.RandomState(2).standard_normal(count) * 10, dtype=torch.float32)
    v[:4] = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 0.0])

    def call(a):
        g('y3_f32_to_bf16', g.ctx, P(a['src']), count, P(a['dst']))
    return run_of([IN('src', v), OUT('dst', (count,), BF16)], call, ['dst'],
                  lambda o: torch.equal(o['dst'], v.to(BF16)) or pytest.fail('not round to nearest even'))


for _n in (4, 4100):
    entry('f32_to_bf16-n%d' % _n, ('y3_f32_to_bf16',), f32_to_bf16, _n)


# ============================================================================================================================
# Unfused graph ops (their first direct tests; exact references) and post-processing.
# ============================================================================================================================
def upsample_nearest(g, n, h, w, c):
    x = np.random.RandomState(h + c).standard_normal((n, h, w, c)).astype(np.float32)

    def call(a):
        g('y3_upsample_nearest', g.ctx, P(a['x']), n, h, w, c, 2 * h, 2 * w, P(a['y']))
    return run_of([IN('x', x), OUT('y', (n, 2 * h, 2 * w, c))], call, ['y'],
                  lambda o: np.testing.assert_array_equal(o['y'].numpy(), np.repeat(np.repeat(x, 2, 1), 2, 2)))


for _a in [(2, 3, 5, 8), (1, 13, 13, 256), (3, 1, 1, 4)]:
    entry('upsample_nearest-%dx%dx%dx%d' % _a, ('y3_upsample_nearest',), upsample_nearest, *_a)


def concat_channels(g, rows, ca, cb):
    rng = np.random.RandomState(rows + ca)
    xa, xb = rng.standard_normal((rows, ca)).astype(np.float32), rng.standard_normal((rows, cb)).astype(np.float32)

    def call(a):
        g('y3_concat_channels', g.ctx, P(a['a']), ca, P(a['b']), cb, rows, P(a['y']))
    return run_of([IN('a', xa), IN('b', xb), OUT('y', (rows, ca + cb))], call, ['y'],
                  lambda o: np.testing.assert_array_equal(o['y'].numpy(), np.concatenate([xa, xb], 1)))


for _a in [(30, 8, 4), (338, 256, 128), (1, 4, 4), (5, 4, 12)]:
    entry('concat_channels-%dx%d+%d' % _a, ('y3_concat_channels',), concat_channels, *_a)


def add(g, count):
    rng = np.random.RandomState(count)
    xa, xb = rng.standard_normal(count).astype(np.float32), rng.standard_normal(count).astype(np.float32)

    def call(a):
        g('y3_add', g.ctx, P(a['a']), P(a['b']), count, P(a['y']))
    return run_of([IN('a', xa), IN('b', xb), OUT('y', (count,))], call, ['y'], lambda o: np.testing.assert_array_equal(o['y'].numpy(), xa + xb))


for _n in (4, 8, 4100, 300004):
    entry('add-n%d' % _n, ('y3_add',), add, _n)


@pytest.mark.gpu
def test_unfused_ops_refuse_channel_counts_that_are_no_multiple_of_four():
    """y3_upsample_nearest, y3_concat_channels and y3_add move 16 bytes per lane (include/yolo355.h): c, ca, cb and count that
    are no multiple of 4 are Y3_EINVAL before any launch - nothing is written, in the outputs or around them."""
    g = G()
    arena = guarded.build(g.dev, [IN('a', np.ones(64, np.float32)), IN('b', np.ones(64, np.float32)), OUT('y', (128,))])
    arena.poison(guarded.POISON_A)
    arena.load()
    a, b, y = P(arena['a']), P(arena['b']), P(arena['y'])
    for name, args in (('y3_upsample_nearest', (a, 1, 2, 2, 7, 4, 4, y)), ('y3_upsample_nearest', (a, 1, 2, 2, 2, 4, 4, y)),
                       ('y3_concat_channels', (a, 7, b, 4, 4, y)), ('y3_concat_channels', (a, 4, b, 5, 4, y)),
                       ('y3_add', (a, b, 7, y)), ('y3_add', (a, b, 1, y)), ('y3_add', (a, b, 0, y))):
        with pytest.raises(ValueError):
            g(name, g.ctx, *args)
    torch.cuda.synchronize()
    arena.check()
    assert bool(torch.isnan(arena['y']).all())


def bn_fold(g, c):
    """scale = gamma * rsqrt(var + eps), shift = beta - mean * scale in fp64, rtol 2e-5 (as the training tests hold the same
    quantities: test_bn_train_stats_and_apply_without_moving_statistics_or_residual)"""
    rng = np.random.RandomState(c)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.3, c).astype(np.float32)
    mean, var = rng.normal(0, 1, c).astype(np.float32), rng.uniform(0.2, 3.0, c).astype(np.float32)
    scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)
    shift = beta.astype(np.float64) - mean.astype(np.float64) * scale

    def call(a):
        t = lambda k: P(a[k])
        g('y3_bn_fold', g.ctx, t('gamma'), t('beta'), t('mean'), t('var'), cf(1e-5), c, t('scale'), t('shift'))

    def verify(o):
        np.testing.assert_allclose(o['scale'].numpy(), scale, rtol=2e-5)
        np.testing.assert_allclose(o['shift'].numpy(), shift, rtol=2e-5, atol=2e-5 * float(np.abs(mean * scale).max()))
    return run_of([IN('gamma', gamma), IN('beta', beta), IN('mean', mean), IN('var', var), OUT('scale', (c,)), OUT('shift', (c,))], call,
                  ['scale', 'shift'], verify)


for _c in (1, 3, 255, 1024):
    entry('bn_fold-c%d' % _c, ('y3_bn_fold',), bn_fold, _c)


def reorg_boxes(g, n, gh, gw, Cn, H, W):
    """test_decode_gpu.box_close against oracle/yolo_ref.reorg_layer"""
    from oracle import yolo_ref
    fm = (np.random.RandomState(1).standard_normal((n, gh, gw, 3 * (5 + Cn))) * 1.5).astype(np.float32)
    ancp = host_f32(COCO_ANCHORS[3:6])
    want = yolo_ref.reorg_layer(fm, COCO_ANCHORS[3:6], [H, W], Cn)[1]

    def call(a):
        g('y3_reorg_boxes', g.ctx, P(a['fm']), n, gh, gw, Cn, H, W, ancp, P(a['boxes']))
    return run_of([IN('fm', fm), OUT('boxes', (n, gh, gw, 3, 4))], call, ['boxes'],
                  lambda o: TD.box_close(o['boxes'].numpy(), want) or pytest.fail('boxes'))


entry('reorg_boxes-2x5x7-c20', ('y3_reorg_boxes',), reorg_boxes, 2, 5, 7, 20, 160, 224)
entry('reorg_boxes-1x13x13-c80', ('y3_reorg_boxes',), reorg_boxes, 1, 13, 13, 80, 416, 416)


def decode(g, n, h, w, Cn, align=16):
    """test_decode_gpu.test_predict_matches_oracle.  align = 4: every pointer at a 4-byte boundary and no more - the header lets
    y3_decode take that (the LDS-staged kernel needs 16-byte alignment; the 4-byte kernel runs instead)."""
    from oracle import yolo_ref
    fms = TD._fms(np.random.RandomState(h + Cn), n, h, w, Cn)
    rb, rc, rp = yolo_ref.predict(fms, COCO_ANCHORS, [h, w], Cn)
    B = 3 * sum((h // s) * (w // s) for s in (32, 16, 8))
    ancp = host_f32(COCO_ANCHORS)
    specs = [IN('fm%d' % (i + 1), f, align=align) for i, f in enumerate(fms)] + [
        OUT('boxes', (n, B, 4), align=align), OUT('confs', (n, B, 1), align=align), OUT('probs', (n, B, Cn), align=align),
        OUT('scores', (n, B, Cn), align=align)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_decode', g.ctx, t('fm1'), t('fm2'), t('fm3'), n, h, w, Cn, ancp, t('boxes'), t('confs'), t('probs'), t('scores'))

    def verify(o):
        assert TD.box_close(o['boxes'].numpy(), rb)
        np.testing.assert_allclose(o['confs'].numpy(), rc, rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(o['probs'].numpy(), rp, rtol=2e-6, atol=2e-7)
        assert torch.equal(o['scores'], o['confs'] * o['probs'])
    return run_of(specs, call, ['boxes', 'confs', 'probs', 'scores'], verify)


for _a in [(1, 64, 32, 1), (2, 64, 96, 80), (1, 96, 64, 252)]:      # 4-byte kernel (C % 4 != 0), LDS-staged, 4-byte (C > 248)
    entry('decode-%dx%dx%d-c%d' % _a, ('y3_decode',), decode, *_a)
entry('decode-2x64x96-c80-align4', ('y3_decode',), decode, 2, 64, 96, 80, align=4)


@functools.lru_cache(maxsize=None)
def _nms_case(mode):
    """test_nms_gpu.test_every_tier_of_candidate_counts: classes in the arg-max, sixteen-wave, sixteen-wave and one-wave tiers"""
    from oracle import nms_ref
    import test_nms_gpu as TN
    boxes, scores = TN.stress_inputs(seed=7, B=20000, C=4)
    scores[:, 0] = 0.5 + 0.5 * scores[:, 0]
    scores[:, 1] = np.where(scores[:, 1] > 0.3, scores[:, 1], 0.1)
    scores[:, 2] = np.where(scores[:, 2] > 0.75, scores[:, 2], 0.1)
    scores[:, 3] = np.where(scores[:, 3] > 0.85, scores[:, 3], 0.1)
    counts = [int((scores[:, c] >= 0.2).sum()) for c in range(4)]
    assert counts[0] > 16384 >= counts[1] > 512 and 16384 >= counts[2] > 512 >= counts[3] > 0, counts
    return boxes, scores, nms_ref.c_per_class(mode, boxes, scores, 4, 40, 0.2, 0.45)


def nms(g, mode):
    """workspace: exactly y3_nms_workspace_bytes; selections bit-exact against the C oracle.  Slots past an image's count are not
    written: they must still hold the poison."""
    boxes, scores, (ob, osc, ol, oi) = _nms_case(mode)
    n, B, Cn, mb = 1, boxes.shape[0], 4, 40
    cap = Cn * mb
    wsb = g.L.y3_nms_workspace_bytes(n, B, Cn, mb)
    m = g._lib.Y3_NMS_TF if mode == 'tf' else g._lib.Y3_NMS_PY
    specs = [IN('boxes', boxes[None]), IN('scores', scores[None]), S('workspace', wsb), OUT('out_boxes', (n, cap, 4)),
             OUT('out_scores', (n, cap)), OUT('out_labels', (n, cap), I32), OUT('out_index', (n, cap), I32), OUT('out_counts', (n,), I32)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_nms', g.ctx, m, t('boxes'), t('scores'), n, B, Cn, mb, cf(0.2), cf(0.45), t('workspace'), ctypes.c_size_t(wsb),
          t('out_boxes'), t('out_scores'), t('out_labels'), t('out_index'), t('out_counts'))

    def view(o, byte):
        k = int(o['out_counts'][0])
        assert k == len(ob)
        out = dict(out_counts=o['out_counts'])
        for name in ('out_boxes', 'out_scores', 'out_labels', 'out_index'):
            assert bool((o[name][0, k:].contiguous().view(U8) == byte).all()), name + ': a slot past the count was written'
            out[name] = o[name][0, :k].contiguous()
        return out

    def verify(o):
        np.testing.assert_array_equal(o['out_index'].numpy(), oi)
        np.testing.assert_array_equal(o['out_labels'].numpy(), ol)
        np.testing.assert_array_equal(o['out_boxes'].numpy(), ob)
        np.testing.assert_array_equal(o['out_scores'].numpy(), osc)
    return run_of(specs, call, ['out_boxes', 'out_scores', 'out_labels', 'out_index', 'out_counts'], verify, view)


for _mode in ('tf', 'py'):
    entry('nms-%s-tiers' % _mode, ('y3_nms',), nms, _mode)


def process_box(g, W, H, Cn):
    """test_next_rows_gpu.test_process_box_batch_on_non_square_images_and_other_class_counts: bit-exact against train_ref"""
    from oracle import train_ref
    rng = np.random.RandomState(W + Cn)
    n, kmax = 4, 10
    boxes, labels, counts = np.zeros((n, kmax, 5), np.float32), np.zeros((n, kmax), np.int64), [3, 0, 10, 6]
    for i, K in enumerate(counts):
        wh, c = rng.uniform(6, 300, (K, 2)), rng.uniform([1, 1], [W - 1, H - 1], (K, 2))
        boxes[i, :K] = np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(0.05, 0.95, (K, 1))], 1)
        labels[i, :K] = rng.randint(0, Cn, K)
    boxes[2, 9] = boxes[2, 3]; boxes[2, 9, 4] = 0.125; labels[2, 9] = (labels[2, 3] + 1) % Cn
    ancp = host_f32(COCO_ANCHORS)
    specs = [IN('boxes', boxes), IN('labels', labels.astype(np.int32)), IN('counts', np.array(counts, np.int32))] + [
        OUT('y_true_%d' % s, (n, H // s, W // s, 3, 6 + Cn)) for s in (32, 16, 8)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_process_box', g.ctx, t('boxes'), t('labels'), t('counts'), n, kmax, Cn, W, H, ancp, t('y_true_32'), t('y_true_16'), t('y_true_8'))

    def verify(o):
        for i, K in enumerate(counts):
            got = [o['y_true_%d' % s][i].numpy() for s in (32, 16, 8)]
            if K == 0:
                assert all((y[..., :-1] == 0).all() and (y[..., -1] == 1).all() for y in got)
                continue
            for y, r in zip(got, train_ref.process_box(boxes[i, :K], labels[i, :K], [W, H], Cn, COCO_ANCHORS)):
                np.testing.assert_array_equal(y, r)
    return run_of(specs, call, ['y_true_32', 'y_true_16', 'y_true_8'], verify)


entry('process_box-64x32-c1', ('y3_process_box',), process_box, 64, 32, 1)
entry('process_box-224x160-c20', ('y3_process_box',), process_box, 224, 160, 20)


def box_iou(g):
    """test_train_gpu.test_box_iou_matches_oracle: rtol 1e-5, atol 1e-6"""
    from oracle import train_ref
    rng = np.random.RandomState(8)
    pred = np.concatenate([rng.uniform(0, 416, (13, 13, 3, 2)), rng.uniform(5, 300, (13, 13, 3, 2))], -1).astype(np.float32)
    gt = np.concatenate([rng.uniform(0, 416, (7, 2)), rng.uniform(5, 300, (7, 2))], -1).astype(np.float32)
    want = train_ref.TrainGraph.box_iou(torch.tensor(pred, dtype=torch.float64), torch.tensor(gt, dtype=torch.float64)).numpy()

    def call(a):
        g('y3_box_iou', g.ctx, P(a['pred_boxes']), 13 * 13 * 3, P(a['true_boxes']), 7, P(a['iou']))
    return run_of([IN('pred_boxes', pred), IN('true_boxes', gt), OUT('iou', (13, 13, 3, 7))], call, ['iou'],
                  lambda o: np.testing.assert_allclose(o['iou'].numpy(), want, rtol=1e-5, atol=1e-6))


entry('box_iou-507x7', ('y3_box_iou',), box_iou)


# ============================================================================================================================
# Device evaluators.  Every table at the alignment the entry documents and checks (f64 and uint64: 8; int32: 4; out_boxes: 16;
# uint8: 1), every scratch at exactly its reported size.  References: voc_cases.assert_table, coco_cases.assert_result,
# beval_cases.reference_of (the gates of the evaluators' own tests).
# ============================================================================================================================
def voc_append(g, case, batch, cap, spare):
    """rows of `batch` images in y3_nms's layout (slots past a count hold NaN / -5) appended to the arena: exact"""
    ids = case.image_ids[:batch]
    (ob, osc, ol, cnt), rows = nms_like(case.preds, ids, cap, 'cpu')
    R = len(rows) + spare
    index = np.arange(len(ids), dtype=np.int32) + 3
    specs = [IN('out_boxes', ob), IN('out_scores', osc, align=4), IN('out_labels', ol, align=4), IN('out_counts', cnt, align=4),
             IN('image_index', index, align=4), OUT('arena_box', (R, 4), F64, align=8), OUT('arena_score', (R,), F64, align=8),
             OUT('arena_label', (R,), I32, align=4), OUT('arena_image', (R,), I32, align=4),
             INOUT('state', np.zeros(2, np.int32), align=4)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_voc_append', g.ctx, t('out_boxes'), t('out_scores'), t('out_labels'), t('out_counts'), t('image_index'), len(ids), cap,
          t('arena_box'), t('arena_score'), t('arena_label'), t('arena_image'), R, t('state'))

    def view(o, byte):
        k = len(rows)
        assert o['state'].tolist() == [k, 0]
        out = dict(state=o['state'])
        for name in ('arena_box', 'arena_score', 'arena_label', 'arena_image'):
            assert bool((o[name][k:].contiguous().view(U8) == byte).all()), name + ': a row past the count was written'
            out[name] = o[name][:k].contiguous()
        return out

    def verify(o):
        pos = {k: i + 3 for i, k in enumerate(ids)}
        np.testing.assert_array_equal(o['arena_box'].numpy(), np.array([r[1:5] for r in rows], np.float32).astype(np.float64).reshape(-1, 4))
        np.testing.assert_array_equal(o['arena_score'].numpy(), np.array([r[5] for r in rows], np.float32).astype(np.float64))
        np.testing.assert_array_equal(o['arena_label'].numpy(), np.array([r[6] for r in rows], np.int32))
        np.testing.assert_array_equal(o['arena_image'].numpy(), np.array([pos[r[0]] for r in rows], np.int32))
    return run_of(specs, call, ['arena_box', 'arena_score', 'arena_label', 'arena_image', 'state'], verify, view)


entry('voc_append-random-5-images', ('y3_voc_append',), voc_append, vc.random_case(1, images=6, classes=3), 5, 48, 7)
entry('voc_append-empty_images', ('y3_voc_append',), voc_append, vc.corner_cases()['empty_images'][0], 3, 4, 0)


def _order(keys, live):
    """rank order by stable sorts, the last key first; dead rows behind every detection"""
    order = np.arange(len(live))
    for key in keys:
        order = order[np.argsort(key[order], kind='stable')]
    return np.concatenate([order[live[order]], order[~live[order]]]).astype(np.int32)


def voc_match_ap(g, case, fn, pad_rows, m07):
    a0 = vc.arena_of(case)
    n, Cn = len(case.preds), case.class_num
    R = n + pad_rows
    pad = lambda x, fill: np.concatenate([x, np.full((pad_rows,) + x.shape[1:], fill, x.dtype)])
    box, score, label, image = pad(a0['box'], 1e9), pad(a0['score'], 2.0), pad(a0['label'], 0), pad(a0['image'], 10 ** 6)
    live = np.arange(R) < n
    order = _order([-score, np.where(live, label, Cn)], live)
    mb, ab = g.L.y3_voc_match_scratch_bytes(R, a0['num_gt']), g.L.y3_voc_ap_scratch_bytes(R)
    thr = (ctypes.c_double * 11)(*np.arange(0., 1.1, 0.1))
    specs = [IN('arena_box', box, align=8), IN('arena_label', label, align=4), IN('arena_image', image, align=4),
             IN('order', order, align=4), IN('n_rows', np.array([n], np.int32), align=4), IN('gt_start', a0['gt_start'], align=4),
             IN('gt_box', a0['gt_box'], align=8), IN('gt_label', a0['gt_label'], align=4), S('match_scratch', mb, align=4),
             S('ap_scratch', ab, align=4), OUT('tp', (R,), U8, align=1), OUT('seg_start', (Cn + 1,), I32, align=4),
             OUT('out', (Cn, 5), F64, align=8)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_voc_match', g.ctx, t('arena_box'), t('arena_label'), t('arena_image'), t('order'), R, t('n_rows'), t('gt_start'),
          t('gt_box'), t('gt_label'), a0['num_images'], a0['num_gt'], Cn, ctypes.c_double(0.5), t('match_scratch'), ctypes.c_size_t(mb),
          t('tp'), t('seg_start'))
        g('y3_voc_ap', g.ctx, t('tp'), t('seg_start'), R, t('gt_label'), a0['num_gt'], Cn, int(m07), thr, t('ap_scratch'),
          ctypes.c_size_t(ab), t('out'))

    def verify(o):
        assert (o['tp'].numpy()[n:] == 0).all()
        vc.assert_table(o['out'].numpy(), vc.reference_table(case, 0.5, m07, fn=fn), m07, 'guarded')
    return run_of(specs, call, ['tp', 'seg_start', 'out'], verify)


for _m07 in (False, True):
    for _name in ('empty_images', 'npos_zero', 'no_second_choice'):
        entry('voc_match_ap-%s-m07_%d' % (_name, _m07), ('y3_voc_match', 'y3_voc_ap'), voc_match_ap, vc.corner_cases()[_name][0], None, 5, _m07)
    entry('voc_match_ap-tied-m07_%d' % _m07, ('y3_voc_match', 'y3_voc_ap'), voc_match_ap, vc.tied_case(), vc.voc_eval_stable, 5, _m07)


def coco(g, case, pad_rows):
    """y3_coco_match -> y3_coco_ap -> y3_coco_summary, each scratch a tensor of its own at exactly its size"""
    from yolov3_tensorflow_amd.utils.eval_utils import COCO_IOU_THRS, COCO_REC_THRS
    a0 = cc.arena_of(case)
    n, Cn, N = len(case.preds), case.class_num, a0['num_images']
    R = n + pad_rows
    pad = lambda x, fill: np.concatenate([x, np.full((pad_rows,) + x.shape[1:], fill, x.dtype)])
    box, score, label, image = pad(a0['box'], 1e9), pad(a0['score'], 2.0), pad(a0['label'], 0), pad(a0['image'], 10 ** 6)
    live = np.arange(R) < n
    order = _order([-score, np.where(live, label, Cn), np.where(live, image, N)], live)
    at = order.astype(np.int64)
    order2 = _order([-score[at], np.where(live[at], label[at], Cn)], live[at])
    mb, ab = g.L.y3_coco_match_scratch_bytes(R, a0['num_gt']), g.L.y3_coco_ap_scratch_bytes(R)
    iou_thrs, rec_thrs = (ctypes.c_double * 10)(*COCO_IOU_THRS), (ctypes.c_double * 101)(*COCO_REC_THRS)
    specs = [IN('arena_box', box, align=8), IN('arena_label', label, align=4), IN('arena_image', image, align=4),
             IN('order', order, align=4), IN('order2', order2, align=4), IN('n_rows', np.array([n], np.int32), align=4),
             IN('gt_start', a0['gt_start'], align=4), IN('gt_box', a0['gt_box'], align=8), IN('gt_label', a0['gt_label'], align=4),
             None if a0['area_scale'] is None else IN('area_scale', a0['area_scale'], align=8),
             S('match_scratch', mb, align=8), S('ap_scratch', ab, align=8), OUT('matched', (R,), I64, align=8),
             OUT('ignored', (R,), I64, align=8), OUT('group_rank', (R,), U8, align=1), OUT('npig', (Cn, 4), I32, align=4),
             OUT('precision', (10, 101, Cn, 4, 3), F64, align=8), OUT('recall', (10, Cn, 4, 3), F64, align=8),
             OUT('per_class', (Cn, 12), F64, align=8), OUT('stats', (12,), F64, align=8)]
    names = [s.name for s in specs if s is not None]

    def call(a):
        t = lambda k: P(a[k]) if k in names else None
        g('y3_coco_match', g.ctx, t('arena_box'), t('arena_label'), t('arena_image'), t('order'), R, t('n_rows'), t('gt_start'),
          t('gt_box'), t('gt_label'), t('area_scale'), N, a0['num_gt'], Cn, iou_thrs, t('match_scratch'), ctypes.c_size_t(mb),
          t('matched'), t('ignored'), t('group_rank'), t('npig'))
        g('y3_coco_ap', g.ctx, t('matched'), t('ignored'), t('group_rank'), t('arena_label'), t('order'), t('order2'), R, t('n_rows'),
          t('npig'), Cn, rec_thrs, t('ap_scratch'), ctypes.c_size_t(ab), t('precision'), t('recall'))
        g('y3_coco_summary', g.ctx, t('precision'), t('recall'), Cn, t('per_class'), t('stats'))

    def view(o, byte):         # ranks at and past the detections' count are no detections: their words are not part of the result
        out = dict(o)
        for k in ('matched', 'ignored', 'group_rank'):
            out[k] = o[k][:n].contiguous()
        return out

    def verify(o):
        cc.assert_result({k: o[k].numpy() for k in ('precision', 'recall', 'per_class', 'stats')}, cc.reference(case), 'guarded')
    return run_of(specs, call, ['matched', 'ignored', 'group_rank', 'npig', 'precision', 'recall', 'per_class', 'stats'], verify, view)


for _name in ('A', 'C', 'D'):
    entry('coco-pin_%s' % _name, ('y3_coco_match', 'y3_coco_ap', 'y3_coco_summary'), coco, cc.pins()[_name][0], 3)
entry('coco-random-4-images', ('y3_coco_match', 'y3_coco_ap', 'y3_coco_summary'), coco, cc.random_case(3, images=4, classes=3, fp32=False), 5)


def batch_eval(g, h, w, Cn, name):
    case = bc.all_cases(h, w, Cn)[name]
    n, cap = case.boxes.shape[0], case.boxes.shape[1]
    gt_cap = case.gt_cap if case.gt_cap is not None else min(bc.cells_of_image(case.h, case.w), 4096)
    sb = g.L.y3_batch_eval_scratch_bytes(n, gt_cap)
    assert sb > 0
    specs = [IN('out_boxes', case.boxes), IN('out_labels', case.labels, align=4), IN('out_counts', np.asarray(case.counts, np.int32), align=4)] + [
        IN('y_true_%d' % (i + 1), y, align=4) for i, y in enumerate(case.y_true)] + [
        S('scratch', sb, align=8), INOUT('table', np.zeros((Cn, 3), np.int64), align=8), INOUT('state', np.zeros(1, np.int32), align=4)]

    def call(a):
        t = lambda k: P(a[k])
        g('y3_batch_eval', g.ctx, t('out_boxes'), t('out_labels'), t('out_counts'), n, cap, t('y_true_1'), t('y_true_2'), t('y_true_3'),
          case.h, case.w, Cn, ctypes.c_double(case.iou_thresh), gt_cap, t('scratch'), ctypes.c_size_t(sb), t('table'), t('state'))

    def verify(o):
        assert int(o['state'][0]) == case.dropped
        if not case.dropped:
            np.testing.assert_array_equal(o['table'].numpy(), bc.reference_of(case))
    return run_of(specs, call, ['table', 'state'], verify)


def _beval_names(h, w, Cn):
    cases = bc.all_cases(h, w, Cn)
    small = sorted(cases, key=lambda k: (cases[k].boxes.size + sum(y.size for y in cases[k].y_true), k))
    return small[:3]


for _h, _w, _c in ((160, 128, 1), (128, 160, 3)):
    for _name in _beval_names(_h, _w, _c):
        entry('batch_eval-%dx%d-c%d-%s' % (_h, _w, _c, _name), ('y3_batch_eval',), batch_eval, _h, _w, _c, _name)


# ============================================================================================================================
# Whole net.  The reference is the same call on plain torch allocations, bit for bit (tests/test_forward_gpu.py and
# tests/test_train_gpu.py hold that call to the oracle).  Parameter buffer and workspaces: exactly their *_bytes, at a 256-byte
# boundary and no more.  The variables themselves are plain device tensors (the net reads them through the host table).
# ============================================================================================================================
NET_DTYPES = {'f32': 0, 'f32_wino': 4, 'bf16': 1}
CLASSES = 80


@functools.lru_cache(maxsize=None)
def _net_host_variables():
    """Per layer: [HWIO kernel, gamma, beta, moving mean, moving variance] or [kernel, bias] (fp32 torch tensors on the host):
    He-scaled kernels, BN parameters and statistics around 1 / 0.  Drawn once, shared by every net case, never modified."""
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, CLASSES, ctypes.byref(h)))      # no context: layer geometry only
    rng = np.random.RandomState(11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    out = []
    for i in range(L.y3_net_num_layers(h)):
        k, s, cin, cout, bn = (ctypes.c_int() for _ in range(5))
        _lib.check(L.y3_net_layer_info(h, i, *[ctypes.byref(v) for v in (k, s, cin, cout, bn)]))
        k, cin, cout = k.value, cin.value, cout.value
        wt = t(rng.standard_normal((k, k, cin, cout)).astype(np.float32) * np.float32(np.sqrt(2.0 / (k * k * cin))))
        if bn.value:
            out.append([wt, t(rng.uniform(0.8, 1.2, cout)), t(rng.normal(0, 0.1, cout)), t(rng.normal(0, 0.1, cout)),
                        t(rng.uniform(0.8, 1.2, cout))])
        else:
            out.append([wt, t(rng.normal(0, 0.1, cout))])
    L.y3_net_destroy(h)
    return out


class _Net(object):
    """A y3_net of the current context bound to device copies of _net_host_variables()."""

    def __init__(self, g, dtype, trainable=False):
        self.g, L = g, g.L
        self.h = ctypes.c_void_p()
        g._lib.check(L.y3_net_create(g.ctx, CLASSES, ctypes.byref(self.h)))
        g._lib.check(L.y3_net_set_dtype(self.h, NET_DTYPES[dtype]))
        host = _net_host_variables()
        self.table = (g._lib.TrainVar * len(host))()
        self.keep, self.moving, off = [], [], 0
        for i, hv in enumerate(host):
            vs = [v.to(g.dev) for v in hv]
            wt, cout = vs[0], int(hv[0].shape[3])
            if len(vs) == 5:
                self.moving += vs[3:]
                ptrs = [v.data_ptr() for v in vs] + [None]
                sizes = [wt.numel(), cout, cout, -1]
            else:
                ptrs = [wt.data_ptr(), None, None, None, None, vs[1].data_ptr()]
                sizes = [wt.numel(), -1, -1, cout]
            offs = []
            for sz in sizes:
                offs.append(off if (trainable and sz >= 0) else -1)
                off += sz if (trainable and sz >= 0) else 0
            self.table[i] = g._lib.TrainVar(*(ptrs + offs + [off if trainable else -1]))
            self.keep.append(vs)
        self.grad_elements = off
        self.moving0 = [m.clone() for m in self.moving]

    def restore_moving(self):
        for m, m0 in zip(self.moving, self.moving0):
            m.copy_(m0)

    def destroy(self):
        self.g.L.y3_net_destroy(self.h)


def net_forward(g, dtype):
    n, h, w = 1, 64, 96                                          # the /32 map is 2 x 3
    L = g.L
    net = _Net(g, dtype)
    pb, wb = L.y3_net_params_bytes(net.h), L.y3_net_workspace_bytes(net.h, n, h, w)
    assert pb > 0 and wb > 0
    x = np.random.RandomState(0).rand(n, h, w, 3).astype(np.float32)
    det = 3 * (5 + CLASSES)
    specs = [IN('x', x), S('params', pb, align=256), S('workspace', wb, align=256)] + [
        OUT('fm%d' % (i + 1), (n, h // s, w // s, det)) for i, s in enumerate((32, 16, 8))]

    def forward(params, ws, xs, fms):
        g('y3_net_set_params', net.h, net.table, P(params), ctypes.c_size_t(pb))
        g('y3_net_forward', net.h, P(xs), n, h, w, P(ws), ctypes.c_size_t(wb), P(fms[0]), P(fms[1]), P(fms[2]))

    def call(a):
        forward(a['params'], a['workspace'], a['x'], [a['fm1'], a['fm2'], a['fm3']])

    def verify(o):
        plain = [torch.empty((n, h // s, w // s, det), device=g.dev) for s in (32, 16, 8)]
        forward(torch.empty(pb, dtype=U8, device=g.dev), torch.empty(wb, dtype=U8, device=g.dev), torch.from_numpy(x).to(g.dev), plain)
        torch.cuda.synchronize()
        for i, p in enumerate(plain):
            assert torch.isfinite(p).all() and float(p.abs().max()) > 0
            assert guarded.bit_identical(o['fm%d' % (i + 1)], p.cpu()), 'fm%d differs from the call on plain allocations' % (i + 1)
        net.destroy()
    return run_of(specs, call, ['fm1', 'fm2', 'fm3'], verify)


for _dt in ('f32', 'f32_wino', 'bf16'):
    entry('net_forward-%s-1x64x96' % _dt, ('y3_net_set_params', 'y3_net_forward'), net_forward, _dt)


def net_train_step(g, dtype):
    from oracle import train_ref
    n, h, w = 2, 64, 96
    L = g.L
    net = _Net(g, dtype, trainable=True)
    wb = L.y3_net_train_workspace_bytes(net.h, net.table, n, h, w)
    assert wb > 0
    x = np.random.RandomState(0).rand(n, h, w, 3).astype(np.float32)
    yts = train_ref.synthetic_targets(9, n, [w, h], CLASSES, COCO_ANCHORS, max_boxes=6)
    ancp = host_f32(COCO_ANCHORS)
    opts = g._lib.TrainOpts(0.9, 0, 0, ctypes.cast(ancp, ctypes.POINTER(ctypes.c_float)))
    specs = [IN('images', x)] + [IN('y_true_%d' % (i + 1), y) for i, y in enumerate(yts)] + [
        OUT('flat_grad', (net.grad_elements,)), S('workspace', wb, align=256), OUT('loss5', (5,))]

    def step(xs, ys, flat, ws, loss5):
        net.restore_moving()
        g('y3_net_train_step', net.h, net.table, P(xs), n, h, w, P(ys[0]), P(ys[1]), P(ys[2]), ctypes.byref(opts), P(flat), P(ws),
          ctypes.c_size_t(wb), P(loss5), g._lib.GradReadyFn(), None)

    def call(a):
        step(a['images'], [a['y_true_1'], a['y_true_2'], a['y_true_3']], a['flat_grad'], a['workspace'], a['loss5'])

    def verify(o):
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(g.dev)
        flat, loss5 = torch.empty(net.grad_elements, device=g.dev), torch.empty(5, device=g.dev)
        step(dev(x), [dev(y) for y in yts], flat, torch.empty(wb, dtype=U8, device=g.dev), loss5)
        torch.cuda.synchronize()
        assert torch.isfinite(flat).all() and torch.isfinite(loss5).all() and float(flat.abs().max()) > 0
        assert guarded.bit_identical(o['loss5'], loss5.cpu()), 'loss5 differs from the call on plain allocations'
        assert guarded.bit_identical(o['flat_grad'], flat.cpu()), 'flat_grad differs from the call on plain allocations'
        net.destroy()
    return run_of(specs, call, ['flat_grad', 'loss5'], verify)


for _dt in ('f32', 'bf16'):
    entry('net_train_step-%s-2x64x96' % _dt, ('y3_net_train_step',), net_train_step, _dt)


def net_train_phases(g, dtype):
    """The same step as its three calls (forward, loss, backward) on the same guarded buffers."""
    from oracle import train_ref
    n, h, w = 2, 64, 96
    L = g.L
    net = _Net(g, dtype, trainable=True)
    wb = L.y3_net_train_workspace_bytes(net.h, net.table, n, h, w)
    assert wb > 0
    x = np.random.RandomState(0).rand(n, h, w, 3).astype(np.float32)
    yts = train_ref.synthetic_targets(9, n, [w, h], CLASSES, COCO_ANCHORS, max_boxes=6)
    ancp = host_f32(COCO_ANCHORS)
    opts = g._lib.TrainOpts(0.9, 0, 0, ctypes.cast(ancp, ctypes.POINTER(ctypes.c_float)))
    specs = [IN('images', x)] + [IN('y_true_%d' % (i + 1), y) for i, y in enumerate(yts)] + [
        OUT('flat_grad', (net.grad_elements,)), S('workspace', wb, align=256), OUT('loss5', (5,))]

    def step(xs, ys, flat, ws, loss5):
        net.restore_moving()
        fms = [ctypes.c_void_p() for _ in range(3)]
        g('y3_net_train_forward', net.h, net.table, P(xs), n, h, w, ctypes.byref(opts), P(ws), ctypes.c_size_t(wb),
          *[ctypes.byref(f) for f in fms])
        lo, hi = ws.data_ptr(), ws.data_ptr() + wb
        assert all(lo <= f.value < hi for f in fms), 'a feature map outside the workspace'
        g('y3_net_train_loss', net.h, P(ys[0]), P(ys[1]), P(ys[2]), ctypes.byref(opts), P(loss5))
        g('y3_net_train_backward', net.h, net.table, P(flat), g._lib.GradReadyFn(), None)

    def call(a):
        step(a['images'], [a['y_true_1'], a['y_true_2'], a['y_true_3']], a['flat_grad'], a['workspace'], a['loss5'])

    def verify(o):
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(g.dev)
        flat, loss5 = torch.empty(net.grad_elements, device=g.dev), torch.empty(5, device=g.dev)
        step(dev(x), [dev(y) for y in yts], flat, torch.empty(wb, dtype=U8, device=g.dev), loss5)
        torch.cuda.synchronize()
        assert torch.isfinite(flat).all() and torch.isfinite(loss5).all() and float(flat.abs().max()) > 0
        assert guarded.bit_identical(o['loss5'], loss5.cpu()), 'loss5 differs from the calls on plain allocations'
        assert guarded.bit_identical(o['flat_grad'], flat.cpu()), 'flat_grad differs from the calls on plain allocations'
        net.destroy()
    return run_of(specs, call, ['flat_grad', 'loss5'], verify)


entry('net_train_phases-f32-2x64x96', ('y3_net_train_forward', 'y3_net_train_loss', 'y3_net_train_backward'), net_train_phases, 'f32')


# ============================================================================================================================
def test_every_entry_point_is_covered_or_excluded():
    """Every _lib.PROTOTYPES entry with a pointer argument is called by a table entry or listed in EXCLUDED with its reason."""
    from yolov3_tensorflow_amd import _lib
    pointer = lambda t: t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)))
    with_pointer = {name for name, (_, args) in _lib.PROTOTYPES.items() if any(pointer(t) for t in args)}
    covered = {name for e in TABLE for name in e.covers}
    assert covered <= with_pointer, sorted(covered - with_pointer)
    assert not (covered & set(EXCLUDED)), sorted(covered & set(EXCLUDED))
    assert set(EXCLUDED) <= with_pointer, sorted(set(EXCLUDED) - with_pointer)
    missing = with_pointer - covered - set(EXCLUDED)
    assert not missing, 'neither in the table nor in EXCLUDED: %s' % sorted(missing)
    assert len({e.id for e in TABLE}) == len(TABLE), 'duplicate entry ids'


@pytest.mark.gpu
@pytest.mark.parametrize('e', TABLE, ids=[e.id for e in TABLE])
def test_guard_bands(e):
    g = G()
    run = e.build(g)
    arena = guarded.build(g.dev, run.specs)
    kept = guarded.run_passes(arena, lambda: run.call(arena), run.outputs, sync=torch.cuda.synchronize)       # poison, call, check guards
    g.fw.check_context()
    assert g.called == set(e.covers), (sorted(g.called), e.covers)
    if run.view is not None:
        kept = [run.view(o, byte) for o, byte in zip(kept, (guarded.POISON_A, guarded.POISON_B))]
    guarded.assert_passes_identical(kept, e.id)
    run.verify(kept[0])


@pytest.mark.gpu
def test_the_harness_detects_on_the_device():
    """tests/test_guarded_cpu.py on device memory, with torch copies standing in for a kernel: a store one element before and
    one element after a tensor is reported; a read one element past an input makes the two passes differ."""
    g = G()
    arena = guarded.build(g.dev, [IN('x', np.arange(8, dtype=np.float32)), OUT('y', (8,)), OUT('m', (1,))])
    x, y, m = arena['x'], arena['y'], arena['m']
    raw = lambda t, lo, hi: arena.buf[t.data_ptr() - arena.base + 4 * lo:t.data_ptr() - arena.base + 4 * hi].view(F32)
    arena.poison(guarded.POISON_A)
    arena.load()
    raw(y, -1, 0).fill_(1.0)
    raw(x, 8, 9).fill_(1.0)
    with pytest.raises(guarded.GuardError) as err:
        arena.check()
    got = sorted((v.name, v.side, v.first, v.last, v.count) for v in err.value.violations)
    assert got == [('x', 'after', 0, 3, 4), ('y', 'before', -4, -1, 4)]
    kept = guarded.run_passes(arena, lambda: m.copy_(raw(x, 0, 9).max().reshape(1)), ['m'], sync=torch.cuda.synchronize)
    assert not guarded.bit_identical(kept[0]['m'], kept[1]['m'])
