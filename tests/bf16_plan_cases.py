"""Helpers of the bf16 inference plan's tests (tests/test_bf16_plan_gpu.py, tests/test_bf16_plan_cpu.py); no conftest.

  * WALK, the input sizes one net handle is walked through, and the data of each;
  * compose_bf16: the bf16 plan (net dtype 1) op by op through the C ABI's per-op entries, driven by the library's exported
    tables (y3_net_layer_info / _graph / _tensor_info / _pool / _fused) and never by the plan's routes;
  * launch_reference: the fp64 result of one launch of that composition from the launch's own inputs as they are on the
    device (tests/test_bf16_gpu.py's ref_conv and bf16_round);
  * misses / tolerance: the gate of that comparison.  The three tolerances are the ones tests/test_bf16_gpu.py states:
      bf16 output      2^-8 |want| + 2e-3     (test_bf16_conv_matches_fp64_on_rounded_operands)
      fp32 output      1e-4 |want| + 2e-3     (the same test, out_f32)
      a fused pair     2^-7 |want| + 2e-2     (test_bf16_fused_stem_and_stride2_conv, test_bf16_fused_first_residual_block)
The part above the GPU section imports neither the device library nor a device."""
import ctypes
import weakref

import numpy as np
import torch
import torch.nn.functional as F

from test_bf16_gpu import bf16_round, ref_conv

# (n, h, w) in walk order: the workspace (6.9, 0.2, 1.8, 2.9, 2.9, 1.5 MB) shrinks, grows, keeps its byte count at another
# layout ((5,64,96) -> (2,96,160)) and shrinks again; 32 x 64 gives maps of 1x2, 2x4 and 4x8
WALK = [(2, 224, 160), (1, 32, 64), (3, 96, 64), (5, 64, 96), (2, 96, 160), (1, 160, 96)]
ARCHS = {'default': 0, 'spp': 1}
TILES = set('Efosx')          # y3_conv_bf16_tile over the layers at every WALK size (35 E, 21 f (SPP 22), 16 o, 1 s, 2 x)
FUSED = [1, 2, 1, 2]          # y3_net_layer_fused of layers 0-3 on the device


def cap_threads():
    torch.set_num_threads(min(torch.get_num_threads(), 16))


# ---- the gate ----------------------------------------------------------------------------------------------------------------
def tolerance(want, kind):
    want = np.abs(np.asarray(want, np.float64))
    if kind == 'bf16':
        return 2.0 ** -8 * want + 2e-3
    if kind == 'f32':
        return 1e-4 * want + 2e-3
    assert kind == 'fused', kind
    return 2.0 ** -7 * want + 2e-2


def misses(got, want, kind):
    """boolean array: the elements of `got` outside the gate (a NaN or an infinity is a miss)"""
    got = np.asarray(got, np.float64)
    return ~(np.abs(got - want) <= tolerance(want, kind))


def upcat(up, x):
    """concat([nearest-neighbour 2x upsample(up), x]) along the channels, as the fused launch reads it"""
    return np.concatenate([np.repeat(np.repeat(up, 2, 1), 2, 2), x], axis=3)


def spp_concat(x):
    """[max13, max9, max5, x] of an NHWC array; max is exact, so on bf16 values this is the pooled tensor bit for bit"""
    t = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    out = torch.cat([F.max_pool2d(t, k, 1, k // 2) for k in (13, 9, 5)] + [t], dim=1)
    return out.permute(0, 2, 3, 1).contiguous().numpy()


def conv_name(i):
    sub, j = ('darknet53_body', i) if i < 52 else ('yolov3_head', i - 52)
    return 'yolov3/%s/%s' % (sub, 'Conv' if j == 0 else 'Conv_%d' % j)


def images(step, n, h, w):
    """structured synthetic images in [0, 1) (conftest.blob_images off the square)"""
    rng = np.random.RandomState(900 + step)
    img = np.zeros((n, h, w, 3), np.float32)
    for g, wt in ((32, 0.45), (8, 0.35), (1, 0.2)):
        t = rng.rand(n, h // g, w // g, 3).astype(np.float32)
        img += wt * np.repeat(np.repeat(t, g, 1), g, 2)
    return img


# ---- GPU section -------------------------------------------------------------------------------------------------------------
def env():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context(), fw.default_device()


def topology(class_num, arch):
    from yolov3_tensorflow_amd import training
    return training._Topology(class_num, arch)


def layer_desc(topo, i, n, h, w):
    """ConvDesc of layer i at input n x h x w from the exported tables: the source tensor's divisor, the up tensor's channels"""
    from yolov3_tensorflow_amd import _lib
    l = topo.layers[i]
    sd = topo.tensors[l['src']]['sdiv']
    c_up = topo.tensors[l['up']]['c'] if l['up'] >= 0 else 0
    return _lib.ConvDesc(n, h // sd, w // sd, l['cin'], c_up, l['cout'], l['k'], l['stride'], l['act'])


def tile_letters(topo, n, h, w):
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    return [chr(L.y3_conv_bf16_tile(ctypes.byref(layer_desc(topo, i, n, h, w)))) for i in range(len(topo.layers))]


class TableNet(object):
    """a net without a context, net dtype 1: the tables and the host queries only"""

    def __init__(self, class_num, arch):
        from yolov3_tensorflow_amd import _lib
        self.L = _lib.lib()
        self.h = ctypes.c_void_p()
        _lib.check(self.L.y3_net_create_arch(None, class_num, arch, ctypes.byref(self.h)))
        _lib.check(self.L.y3_net_set_dtype(self.h, 1))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.y3_net_destroy(self.h)

    def fused(self, n, h, w):
        return [self.L.y3_net_layer_fused(self.h, i, n, h, w) for i in range(self.L.y3_net_num_layers(self.h))]

    def pools(self):
        return [self.L.y3_net_layer_pool(self.h, i) for i in range(self.L.y3_net_num_layers(self.h))]

    def workspace_bytes(self, n, h, w):
        return self.L.y3_net_workspace_bytes(self.h, n, h, w)


_PARAMS = weakref.WeakKeyDictionary()      # model -> per layer: HWIO variable, packed bf16 kernel, scale, shift


def layer_params(model, topo):
    """per layer: w (the HWIO fp32 variable's tensor), wp (y3_pack_conv_weights_bf16 of it; None for the Cin = 3 stem, which
    reads the HWIO kernel), scale / shift of engine.prepare_conv_params (detection convs: ones and the bias).  Packed once
    per model; call under the model's graph."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import engine
    if model in _PARAMS:
        return _PARAMS[model]
    fw, _lib, L, ctx, dev = env()
    variables = {v.op_name: v for v in y3.global_variables(scope='yolov3')}
    out = []
    for i, l in enumerate(topo.layers):
        base = conv_name(i)
        bn = tuple(variables['%s/BatchNorm/%s' % (base, s)] for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')) \
            if l['bn'] else None
        _, scale, shift = engine.prepare_conv_params(variables[base + '/weights'], bn_vars=bn,
                                                     bias_var=None if l['bn'] else variables[base + '/biases'])
        wt = variables[base + '/weights'].tensor
        assert tuple(wt.shape) == (l['k'], l['k'], l['cin'], l['cout']), (i, tuple(wt.shape))
        wp = None
        if l['cin'] != 3:
            wp = torch.empty(l['k'] * l['k'] * l['cin'] * l['cout'], dtype=torch.bfloat16, device=dev)
            _lib.check(L.y3_pack_conv_weights_bf16(ctx, fw.ptr(wt), l['k'], l['cin'], l['cout'], fw.ptr(wp)))
        out.append(dict(w=wt, wp=wp, scale=scale, shift=shift))
    _PARAMS[model] = out
    return out


def compose_bf16(model, x, arch):
    """The bf16 plan op by op.  Per launch that y3_net_layer_fused reports at this size the per-op entry: flags 1, 2 at layers
    0 / 1 one y3_conv2d_fwd_bf16_stem_s2 (fp32 image, the stem's fp32 HWIO kernel, layer 1's packed kernel), at layers 2 / 3 one
    y3_resblock64_fwd_bf16, else y3_conv2d_fwd_bf16 on a ConvDesc of the tensors' actual shapes (x_up / c_up, the residual,
    out_f32 = 1 and act = 0 into an external feature map, the unfused Cin = 3 stem on the fp32 image and the HWIO kernel), with
    y3_spp_fwd (half = 1) in front of the pool layer.  x: [n, h, w, 3] fp32 on the device; call under the model's graph.
    Returns (tensors by tensor id, [fm1, fm2, fm3], launches); a launch: dict(kind 'stem_s2' | 'resblock64' | 'conv', layers,
    src / up / resid / dst tensor ids, pooled (the device's spp(src)) or None, out_f32, tile).  Every device buffer stays
    referenced from what is returned."""
    fw, _lib, L, ctx, dev = env()
    topo = topology(model.class_num, arch)
    n, h, w, _ = x.shape
    P = layer_params(model, topo)
    with TableNet(model.class_num, arch) as tn:
        flags, pools = tn.fused(n, h, w), tn.pools()
    letters = tile_letters(topo, n, h, w)
    tens, outs, launches = {0: x}, {}, []
    nl = len(topo.layers)
    i = 0
    while i < nl:
        l, p = topo.layers[i], P[i]
        if flags[i] == 1:
            assert i in (0, 2) and flags[i + 1] == 2, flags[:i + 2]
            l1, p1 = topo.layers[i + 1], P[i + 1]
            src = tens[l['src']]
            assert l1['src'] == l['dst']
            if i == 0:
                y = torch.empty((n, h // 2, w // 2, l1['cout']), dtype=torch.bfloat16, device=dev)
                _lib.check(L.y3_conv2d_fwd_bf16_stem_s2(ctx, n, h, w, fw.ptr(src), fw.ptr(p['w']), fw.ptr(p['scale']), fw.ptr(p['shift']),
                                                        fw.ptr(p1['wp']), fw.ptr(p1['scale']), fw.ptr(p1['shift']), fw.ptr(y)))
                kind = 'stem_s2'
            else:
                assert l1['resid'] == l['src']
                y = torch.empty(tuple(src.shape[:3]) + (l1['cout'],), dtype=torch.bfloat16, device=dev)
                _lib.check(L.y3_resblock64_fwd_bf16(ctx, n, src.shape[1], src.shape[2], fw.ptr(src), fw.ptr(p['wp']), fw.ptr(p['scale']),
                                                    fw.ptr(p['shift']), fw.ptr(p1['wp']), fw.ptr(p1['scale']), fw.ptr(p1['shift']),
                                                    fw.ptr(y)))
                kind = 'resblock64'
            tens[l1['dst']] = y
            launches.append(dict(kind=kind, layers=(i, i + 1), src=l['src'], up=-1, resid=l1['resid'], dst=l1['dst'], pooled=None,
                                 out_f32=0, tile=letters[i] + letters[i + 1]))
            i += 2
            continue
        assert flags[i] == 0, (i, flags[i])
        src = tens[l['src']]
        pooled = None
        if pools[i]:
            pooled = torch.empty(tuple(src.shape[:3]) + (4 * src.shape[3],), dtype=src.dtype, device=dev)
            _lib.check(L.y3_spp_fwd(ctx, fw.ptr(src), 1, n, src.shape[1], src.shape[2], src.shape[3], fw.ptr(pooled)))
            src = pooled
        up = tens[l['up']] if l['up'] >= 0 else None
        res = tens[l['resid']] if l['resid'] >= 0 else None
        ext = topo.tensors[l['dst']]['ext']
        out_f32 = 1 if ext >= 0 else 0
        d = _lib.ConvDesc(n, src.shape[1], src.shape[2], l['cin'], up.shape[3] if up is not None else 0, l['cout'], l['k'],
                          l['stride'], 0 if out_f32 else l['act'])
        assert d.cin == src.shape[3] + d.c_up, (i, d.cin, tuple(src.shape), d.c_up)
        y = torch.empty((n, src.shape[1] // l['stride'], src.shape[2] // l['stride'], l['cout']),
                        dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
        _lib.check(L.y3_conv2d_fwd_bf16(ctx, ctypes.byref(d), fw.ptr(src), fw.ptr(up), fw.ptr(p['w'] if l['cin'] == 3 else p['wp']),
                                        fw.ptr(p['scale']), fw.ptr(p['shift']), fw.ptr(res), fw.ptr(y), out_f32))
        tens[l['dst']] = y
        if ext >= 0:
            outs[ext] = y
        launches.append(dict(kind='conv', layers=(i,), src=l['src'], up=l['up'], resid=l['resid'], dst=l['dst'], pooled=pooled,
                             out_f32=out_f32, tile=chr(L.y3_conv_bf16_tile(ctypes.byref(d)))))
        i += 1
    torch.cuda.synchronize()
    fw.check_context()
    return tens, [outs[0], outs[1], outs[2]], launches


def _np(t):
    return t.float().cpu().numpy()


def launch_reference(launch, tens, P, topo):
    """(want fp64, gate kind) of one launch from its own inputs as they are on the device: the bf16 tensors' values exactly,
    the packed kernels' bf16 values (the pack rounds the variable to nearest even, as torch does), fp32 scale / shift.
    What is rounded besides: the tensor between the two convs of a fused pair, to bf16, as the kernels do (the fused stem
    rounds neither the fp32 image nor its fp32 kernel: it splits each into two bf16 parts; conv_stem_bf16_kernel runs in
    fp32).  The upsample + concat and the SPP concat are materialised here."""
    wq = lambda i: P[i]['w'].to(torch.bfloat16).float().cpu().numpy()      # the kernel's bf16 values, HWIO
    sc = lambda i: (P[i]['scale'].cpu().numpy(), P[i]['shift'].cpu().numpy())
    src = _np(tens[launch['src']])
    if launch['kind'] == 'stem_s2':
        i0, i1 = launch['layers']
        mid = bf16_round(ref_conv(src, P[i0]['w'].cpu().numpy(), *sc(i0), 3, 1, True))
        return ref_conv(mid, wq(i1), *sc(i1), 3, 2, True), 'fused'
    if launch['kind'] == 'resblock64':
        i2, i3 = launch['layers']
        mid = bf16_round(ref_conv(src, wq(i2), *sc(i2), 1, 1, True))
        return ref_conv(mid, wq(i3), *sc(i3), 3, 1, True, src), 'fused'
    i, = launch['layers']
    l = topo.layers[i]
    if launch['pooled'] is not None:
        want_pooled = spp_concat(src)
        assert np.array_equal(_np(launch['pooled']), want_pooled), 'layer %d: the pooled tensor is not spp(src)' % i
        src = want_pooled
    if launch['up'] >= 0:
        src = upcat(_np(tens[launch['up']]), src)
    res = _np(tens[launch['resid']]) if launch['resid'] >= 0 else None
    wt = P[i]['w'].cpu().numpy() if l['cin'] == 3 else wq(i)
    want = ref_conv(src, wt, *sc(i), l['k'], l['stride'], bool(l['act']) and not launch['out_f32'], res)
    return want, 'f32' if launch['out_f32'] else 'bf16'


def describe_miss(launch, topo, got, want, kind):
    """layer index, its (k, stride, cin, cout), the tile letter, the worst element's coordinates"""
    err = np.abs(np.asarray(got, np.float64) - want) / tolerance(want, kind)
    err = np.where(np.isfinite(err), err, np.inf)
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    what = ['layer %d (k, stride, cin, cout) = %s' % (i, tuple(topo.layers[i][s] for s in ('k', 'stride', 'cin', 'cout')))
            for i in launch['layers']]
    return '%s %s, tile %s: %d of %d elements outside the %s gate; worst at (n, y, x, c) = %s: got %r, want %r, tolerance %.3e' % (
        launch['kind'], ' + '.join(what), launch['tile'], int(misses(got, want, kind).sum()), err.size, kind, tuple(int(v) for v in at),
        float(np.asarray(got)[at]), float(want[at]), float(tolerance(want, kind)[at]))
