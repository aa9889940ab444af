"""Oracle pieces and cases of the SPP tests (tests/test_spp_cpu.py, tests/test_spp_gpu.py).  The definition is the comment
under "SPP" in include/yolo355.h: spp(x) = concat([mp_13, mp_9, mp_5, x]) over NHWC maps, backward to the first maximum of
every window in row-major order, summed per input element in a fixed order.

  spp_ref            the op with torch F.max_pool2d(x, k, 1, k // 2)
  first_argmax       the first-max rule in numpy (the window scanned y ascending, then x ascending, a later value wins only
                     if it is greater)
  bwd_ordered        the fp32 sum in the stated order: identity, then k = 5, 9, 13, within a k the q in row-major order
  bwd_fp64           torch fp64 autograd of spp_ref, and the sum of the |terms| that reach each element
  spp_params         the oracle's synthetic parameters for the 76-conv graph (one more 1x1 conv at head position 3)
  forward_spp        the inference forward, composed from oracle.yolo_ref's graph functions
  SppTrainGraph      oracle.train_ref.TrainGraph with the SPP _yolo_block for f = 512
  train_step         train_ref.train_step's twin on that graph
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import train_ref, yolo_ref

WINDOWS = (5, 9, 13)            # backward's order
SLOT = {13: 0, 9: 1, 5: 2}      # spp(x) = [mp_13, mp_9, mp_5, x]
MAX_TERMS = 1 + 25 + 81 + 169   # gradients that can reach one input element

CPU_SHAPES = [(1, 1, 1, 8), (2, 3, 4, 8), (2, 7, 5, 16), (1, 13, 13, 8), (1, 19, 20, 8)]
# (1,40,33,16): more than one tile a side in both kernels; 520 channels: a last chunk that is not full.  The two after it are
# not the issue's: a map cut on one axis only (40 rows, 13 columns in one tile), and sides of 33 and 32 - the first size that
# is cut next to the last that is one tile
GPU_SHAPES = [(1, 1, 1, 8), (2, 3, 4, 8), (2, 7, 5, 520), (1, 13, 13, 512), (1, 19, 19, 512), (1, 40, 33, 16), (1, 40, 13, 8),
              (2, 33, 32, 8)]


def inputs(kind, shape, seed):
    """x [n,h,w,c] float32, every value exact in bf16.  'continuous': normal draws rounded to bf16 (ties are rare);
    'ties': drawn from {-1, 0, 0.5, 1}, so that most windows hold their maximum several times."""
    rng = np.random.RandomState(seed)
    if kind == 'ties':
        return rng.choice(np.array([-1.0, 0.0, 0.5, 1.0], np.float32), size=shape).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    return x.to(torch.bfloat16).to(torch.float32).numpy()


def gradients(shape, seed):
    n, h, w, c = shape
    return np.random.RandomState(seed).standard_normal((n, h, w, 4 * c)).astype(np.float32)


def spp_ref(x):
    """x: NHWC torch tensor (any float dtype; bf16 is pooled as fp32, which is exact) -> [n,h,w,4c] of the same dtype"""
    t = x.to(torch.float32 if x.dtype == torch.bfloat16 else x.dtype).permute(0, 3, 1, 2)
    out = torch.cat([F.max_pool2d(t, k, 1, k // 2) for k in (13, 9, 5)] + [t], dim=1)
    return out.permute(0, 2, 3, 1).contiguous().to(x.dtype)


def first_argmax(x, k):
    """x [n,h,w,c] -> (ay, ax) int arrays [n,h,w,c]: the first position of each k x k window, row-major, whose value is the
    window's maximum (positions outside the map are left out); compared in x's own precision"""
    x = np.asarray(x)
    n, h, w, c = x.shape
    r = k // 2
    pad = np.full((n, h + 2 * r, w + 2 * r, c), -np.inf, x.dtype)
    pad[:, r:r + h, r:r + w] = x
    m = np.full(x.shape, -np.inf, x.dtype)
    ay = np.full(x.shape, -1, np.int64)
    ax = np.full(x.shape, -1, np.int64)
    ys = np.arange(h).reshape(1, h, 1, 1)
    xs = np.arange(w).reshape(1, 1, w, 1)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            v = pad[:, r + dy:r + dy + h, r + dx:r + dx + w]
            take = v > m
            m = np.where(take, v, m)
            ay = np.where(take, ys + dy, ay)
            ax = np.where(take, xs + dx, ax)
    return ay, ax


def bwd_ordered(x, g, dx0=None, argmax=None):
    """dx [n,h,w,c] float32: per element g[p, 3c + ch], then + g[q, slot(k) c + ch] for k = 5, 9, 13 and, within a k, every q in
    row-major order whose window's first maximum is p - one rounded fp32 addition per term; dx0: what dx held (accumulate).
    argmax: {k: (ay, ax)} to use instead of first_argmax(x, k)."""
    x = np.asarray(x, np.float32)
    g = np.asarray(g, np.float32)
    n, h, w, c = x.shape
    acc = g[..., 3 * c:].copy()
    ys = np.arange(h).reshape(1, h, 1, 1)
    xs = np.arange(w).reshape(1, 1, w, 1)
    for k in WINDOWS:
        r = k // 2
        ay, ax = argmax[k] if argmax is not None else first_argmax(x, k)
        pay = np.full((n, h + 2 * r, w + 2 * r, c), -1, np.int64)
        pax = pay.copy()
        pg = np.zeros((n, h + 2 * r, w + 2 * r, c), np.float32)
        pay[:, r:r + h, r:r + w] = ay
        pax[:, r:r + h, r:r + w] = ax
        pg[:, r:r + h, r:r + w] = g[..., SLOT[k] * c:(SLOT[k] + 1) * c]
        for dy in range(-r, r + 1):          # q = p + (dy, dx): row-major in q for every p at once
            for dx in range(-r, r + 1):
                sl = (slice(None), slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
                hit = (pay[sl] == ys) & (pax[sl] == xs)
                acc = np.where(hit, (acc + pg[sl]).astype(np.float32), acc)
    return acc if dx0 is None else (np.asarray(dx0, np.float32) + acc).astype(np.float32)


def bwd_fp64(x, g):
    """(dx, sum of |terms|) of torch's fp64 autograd through spp_ref: [n,h,w,c] float64 each"""
    out = []
    for gg in (np.asarray(g, np.float64), np.abs(np.asarray(g, np.float64))):
        t = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
        spp_ref(t).backward(torch.from_numpy(gg))
        out.append(t.grad.numpy())
    return out[0], out[1]


# ---- the 76-conv graph -------------------------------------------------------------------------------------------------
SPP_HEAD_CONV = 3            # head position of the added 1x1 conv (layer 55): reads spp(Conv_2), 2048 -> 512


def _head_index(name):
    conv = name.split('/')[2]
    return 0 if conv == 'Conv' else int(conv.split('_')[1])


def _head_name(prefix, j, leaf):
    return '%s/yolov3_head/%s/%s' % (prefix, 'Conv' if j == 0 else 'Conv_%d' % j, leaf)


def spp_params(class_num=80, seed=1, prefix='yolov3'):
    """yolo_ref.synthetic_params for the SPP graph, in creation order: the default graph's values with the head names from
    position 3 on shifted by one, and the added conv drawn the same way from a generator of its own."""
    base = yolo_ref.synthetic_params(class_num, seed, prefix)
    rng = np.random.RandomState([seed, 0x737070])
    added = OrderedDict()
    added['weights'] = rng.normal(0.0, np.sqrt(2.0 / 2048), size=(1, 1, 2048, 512)).astype(np.float32)
    added['BatchNorm/gamma'] = rng.uniform(0.8, 1.2, size=(512,)).astype(np.float32)
    added['BatchNorm/beta'] = rng.normal(0.0, 0.05, size=(512,)).astype(np.float32)
    added['BatchNorm/moving_mean'] = rng.normal(0.0, 0.05, size=(512,)).astype(np.float32)
    added['BatchNorm/moving_variance'] = rng.uniform(0.8, 1.2, size=(512,)).astype(np.float32)
    out = OrderedDict()
    done = False
    for name, v in base.items():
        parts = name.split('/')
        if parts[1] != 'yolov3_head' or _head_index(name) < SPP_HEAD_CONV:
            out[name] = v
            continue
        if not done:
            for leaf, a in added.items():
                out[_head_name(prefix, SPP_HEAD_CONV, leaf)] = a
            done = True
        out[_head_name(prefix, _head_index(name) + 1, '/'.join(parts[3:]))] = v
    return out


def forward_spp(params, x_nhwc, class_num=80, dtype=torch.float32, prefix='yolov3'):
    """yolo_ref.forward for the SPP architecture, from the same graph functions: three NHWC numpy feature maps"""
    b = yolo_ref._Builder(params, prefix, dtype)
    x = torch.from_numpy(np.asarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2).contiguous()
    det = 3 * (5 + class_num)
    with torch.no_grad():
        b.enter('darknet53_body')
        route_1, route_2, route_3 = yolo_ref.darknet53_body(b, x)
        b.enter('yolov3_head')
        net = yolo_ref.conv2d(b, route_3, 512, 1)
        net = yolo_ref.conv2d(b, net, 1024, 3)
        net = yolo_ref.conv2d(b, net, 512, 1)
        net = torch.cat([F.max_pool2d(net, k, 1, k // 2) for k in (13, 9, 5)] + [net], dim=1)
        net = yolo_ref.conv2d(b, net, 512, 1)
        net = yolo_ref.conv2d(b, net, 1024, 3)
        inter1 = yolo_ref.conv2d(b, net, 512, 1)
        net = yolo_ref.conv2d(b, inter1, 1024, 3)
        fm1 = yolo_ref._slim_conv(b, net, det, 1, 1, 'SAME', bn=False, act=False)
        inter1 = yolo_ref.upsample_layer(yolo_ref.conv2d(b, inter1, 256, 1), route_2.shape[2:])
        inter2, net = yolo_ref.yolo_block(b, torch.cat([inter1, route_2], dim=1), 256)
        fm2 = yolo_ref._slim_conv(b, net, det, 1, 1, 'SAME', bn=False, act=False)
        inter2 = yolo_ref.upsample_layer(yolo_ref.conv2d(b, inter2, 128, 1), route_1.shape[2:])
        _, fm3 = yolo_ref.yolo_block(b, torch.cat([inter2, route_1], dim=1), 128)
        fm3 = yolo_ref._slim_conv(b, fm3, det, 1, 1, 'SAME', bn=False, act=False)
    return tuple(f.permute(0, 2, 3, 1).contiguous().numpy() for f in (fm1, fm2, fm3))


class SppMixin(object):
    """The SPP block in the f = 512 yolo_block of a train_ref.TrainGraph (or a subclass of it: mix in first).  pool_argmax, set
    after construction: optional {k: (ay, ax)} NHWC index arrays - the window maxima are then read at these positions (a
    gather, so the gradient goes exactly there) instead of taken by this graph's own comparison: a near-tie that two
    implementations resolve differently moves a whole gradient entry, the LeakyReLU reason of TrainGraph.masks."""
    pool_argmax = None
    pool_input = None

    def _spp(self, x):
        self.pool_input = x.detach()
        n, c, h, w = x.shape
        parts = []
        for k in (13, 9, 5):
            if self.pool_argmax is None:
                parts.append(F.max_pool2d(x, k, 1, k // 2))
                continue
            ay, ax = (torch.as_tensor(np.asarray(a)).permute(0, 3, 1, 2) for a in self.pool_argmax[k])
            flat = (ay * w + ax).reshape(n, c, h * w)
            parts.append(x.reshape(n, c, h * w).gather(2, flat).reshape(n, c, h, w))
        return torch.cat(parts + [x], dim=1)

    def _yolo_block(self, x, f):
        if f != 512:
            return train_ref.TrainGraph._yolo_block(self, x, f)
        x = self._conv(x, 512, 1)
        x = self._conv(x, 1024, 3)
        x = self._conv(x, 512, 1)
        x = self._spp(x)
        x = self._conv(x, 512, 1)
        x = self._conv(x, 1024, 3)
        x = self._conv(x, 512, 1)
        return x, self._conv(x, 1024, 3)


class SppTrainGraph(SppMixin, train_ref.TrainGraph):
    pass


def train_step(params, x, y_trues, anchors, class_num=80, optimizer='sgd', lr=1e-4, weight_decay=5e-4, bn_decay=0.99,
               clip=100.0, update_names=None, dtype=torch.float64, step=1, masks=None, pool_argmax=None):
    """train_ref.train_step on SppTrainGraph.  update_names: the trainable variable names to differentiate (None: all)."""
    g = SppTrainGraph(params, class_num, dtype, masks=masks)
    g.pool_argmax = pool_argmax
    g.iou_margins = []          # per scale: the smallest |best IoU - 0.5| (train_ref.train_step's iou_margins)
    fms = g.forward(x)
    loss = g.compute_loss(fms, y_trues, anchors)
    l2 = g.l2_loss(weight_decay)
    total = loss[0] + l2
    names = [k for k, v in g.p.items() if v.requires_grad and (update_names is None or k in update_names)]
    grads = torch.autograd.grad(total, [g.p[k] for k in names], allow_unused=True)
    new_params = OrderedDict((k, v.detach().clone()) for k, v in g.p.items())
    out_grads = OrderedDict()
    for k, gr in zip(names, grads):
        if gr is None:
            continue
        gc = train_ref.clip_by_norm(gr, clip)
        out_grads[k] = gc.numpy()
        new_params[k] = train_ref.apply_update(optimizer, g.p[k].detach(), gc, {}, lr, step)
    for name, (mean, var_b, var_u) in g.batch_stats.items():
        mm, mv = name + '/BatchNorm/moving_mean', name + '/BatchNorm/moving_variance'
        new_params[mm] = g.p[mm] * bn_decay + mean * (1 - bn_decay)
        new_params[mv] = g.p[mv] * bn_decay + var_u * (1 - bn_decay)
    return dict(loss=[float(v.detach()) for v in loss], l2=float(l2.detach()), grads=out_grads,
                new_params=OrderedDict((k, v.numpy()) for k, v in new_params.items()), graph=g,
                iou_margins=list(g.iou_margins))


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  The two SPP
# entry points are added from here, as mosaic_cases.py and layerwise_cases.py add theirs: this module is imported whenever the
# suite is collected.  tests/test_spp_gpu.py runs the entries through that module's own test.
GUARD_SHAPES = [(2, 7, 5, 520), (1, 13, 13, 512)]


def _register_guard_band_entries():
    import ctypes
    import test_guard_bands_gpu as TG
    if 'y3_net_create_arch' in TG.EXCLUDED:
        return
    TG.EXCLUDED.update({'y3_net_create_arch': 'net handle', 'y3_net_arch': 'net handle', 'y3_net_layer_pool': 'net handle',
                        'y3_net_train_saved_pool': 'net handle, host pointer'})

    def spp_fwd(g, shape, bf16):
        n, h, w, c = shape
        dt = torch.bfloat16 if bf16 else torch.float32
        x = torch.from_numpy(inputs('ties' if bf16 else 'continuous', shape, seed=31)).to(dt)
        specs = [TG.IN('x', x), TG.OUT('out', (n, h, w, 4 * c), dtype=dt)]

        def call(a):
            g('y3_spp_fwd', g.ctx, TG.P(a['x']), int(bf16), n, h, w, c, TG.P(a['out']))

        def verify(o):
            assert TG.guarded.bit_identical(o['out'], spp_ref(x))
        return TG.run_of(specs, call, ['out'], verify)

    def spp_bwd(g, shape, bf16, accumulate):
        """x is the last slot of a materialised spp(x) of exactly its own size: stride 4c, nothing behind the last row"""
        n, h, w, c = shape
        dt = torch.bfloat16 if bf16 else torch.float32
        xn = inputs('ties', shape, seed=32)
        gn = gradients(shape, seed=33)
        dx0 = np.random.RandomState(34).standard_normal(shape).astype(np.float32)
        pooled = spp_ref(torch.from_numpy(xn)).to(dt)
        specs = [TG.IN('pooled', pooled), TG.IN('g', gn), TG.INOUT('dx', dx0) if accumulate else TG.OUT('dx', shape)]

        def call(a):
            x = ctypes.c_void_p(a['pooled'].data_ptr() + 3 * c * pooled.element_size())
            g('y3_spp_bwd', g.ctx, x, 4 * c, int(bf16), TG.P(a['g']), n, h, w, c, int(accumulate), TG.P(a['dx']))

        def verify(o):
            want = bwd_ordered(xn, gn, dx0 if accumulate else None)
            assert TG.guarded.bit_identical(o['dx'], torch.from_numpy(want))
        return TG.run_of(specs, call, ['dx'], verify)

    for shape in GUARD_SHAPES:
        tag = 'x'.join(str(v) for v in shape)
        for bf16 in (False, True):
            TG.entry('spp_fwd-%s-%s' % (tag, 'bf16' if bf16 else 'f32'), ('y3_spp_fwd',), spp_fwd, shape, bf16)
        TG.entry('spp_bwd-%s-f32' % tag, ('y3_spp_bwd',), spp_bwd, shape, False, False)
        TG.entry('spp_bwd-%s-bf16-accumulate' % tag, ('y3_spp_bwd',), spp_bwd, shape, True, True)
    # (mosaic_cases.py: when this module is imported before pytest has read test_guard_bands' parametrize mark, whose list of ids
    # was made when that module was imported, the new entries need their ids there; imported later, nothing changes)
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entries()
