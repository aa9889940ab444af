"""The layer-wise update rules (include/yolo355.h, "Layer-wise update rules": AdamW, LARS, LAMB) in numpy, written from that
comment block and nothing else; their perturbed forms; the inputs the kernel tests share.  Used by
test_layerwise_update_cpu.py and test_layerwise_update_gpu.py.

    evaluate(kind, tensor, hp, dtype)      the rule (fp64 is the reference; float32 measures what fp32 arithmetic costs)
    restated(kind, tensor, hp, perturb)    the rule again in fp64 with ONE thing changed (None: nothing, and then it is
                                           evaluate's result bit for bit - test_layerwise_update_cpu.py holds it to that)
"""
import ctypes

import numpy as np

KINDS = ('adamw', 'lars', 'lamb')
KIND_ID = dict(adamw=4, lars=5, lamb=6)             # Y3_OPT_ADAMW / _LARS / _LAMB
NO_ADAPT = 1                                        # Y3_PARAM_NO_ADAPT
SLOTS = dict(adamw=2, lars=1, lamb=2)
TOL = 2e-6                     # of each output tensor's max |expected| (test_optimizer_gpu.TOL)
GUARD = 100.0                  # a perturbed rule must be more than GUARD tolerances away
OUTPUTS = ('w', 'g', 's0', 's1', 'ratio')
F32 = lambda x: float(np.float32(x))

# which perturbed rule each kind's tests would catch
GUARDS = dict(adamw=('l2_in_gradient',),
              lars=('l2_in_gradient', 'no_trust_ratio', 'ratio_outside_accumulator', 'flag_ignored', 'w_norm_after_step'),
              lamb=('l2_in_gradient', 'no_trust_ratio', 'flag_ignored', 'bias_correction_dropped', 'w_norm_after_step'))

# ---- inputs ---------------------------------------------------------------------------------------------------------------
# 7, 255: n % 4 != 0 (one element per lane); 8192: exactly one chunk; 8193: one element per lane across a chunk edge; 8196:
# four per lane, last chunk of one float4; 18, 1024; 300000: 37 chunks.  Then 4096 elements of w = 0 and 4096 of g = 0.
SIZES = (7, 255, 8192, 8193, 8196, 18, 1024, 300000, 4096, 4096)
ZERO_W, ZERO_G = 8, 9
LAMBDA = (0.0, 5e-2, 5e-2, 0.0, 5e-2, 0.0, 5e-2, 5e-2, 5e-2, 0.0)
NORM = (300.0, 30.0, 30.0, 300.0, 300.0, 30.0, 30.0, 300.0, 30.0, 0.0)       # of grad_scale * g: above / below the clip norm
FLAGS = (0, NO_ADAPT, 0, 0, 0, 0, NO_ADAPT, 0, 0, 0)
NO_SHADOW = (3,)                                    # a NULL entry of the shadow array
STEP = 3                                            # the t of the bias corrections
_BASE = dict(grad_scale=0.5, clip_norm=100.0, lr=5e-2, momentum=0.8, beta1=0.9, beta2=0.999, trust=0.02, ema_step=0.1)
_EPS = dict(adamw=1e-8, lars=0.0, lamb=1e-6)


def hyper(kind, step=STEP, **over):
    """The twelve floats of y3_layerwise_hp at their float32 values: the host forms lr_t, bias1 and bias2 in double from the
    float32 betas, then the ABI rounds them once."""
    hp = dict(_BASE, eps=_EPS[kind])
    hp.update(over)
    lr = float(hp['lr'])                                # (the double the host's schedule gave)
    hp = {k: F32(v) for k, v in hp.items()}
    b1, b2 = hp['beta1'], hp['beta2']
    adaptive = kind != 'lars'
    hp['lr_t'] = F32(lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)) if adaptive else hp['lr']
    hp['bias1'] = F32(1.0 / (1.0 - b1 ** step)) if adaptive else 1.0
    hp['bias2'] = F32(1.0 / (1.0 - b2 ** step)) if adaptive else 1.0
    return hp


HP_FIELDS = ('grad_scale', 'clip_norm', 'lr', 'lr_t', 'momentum', 'beta1', 'beta2', 'eps', 'bias1', 'bias2', 'trust', 'ema_step')


def hp_struct(hp):
    from yolov3_tensorflow_amd import _lib
    return _lib.LayerwiseHp(**{k: hp[k] for k in HP_FIELDS})


_CACHE = {}


def inputs(kind):
    """One list of tensors per kind (numpy float32): w, g, warm non-zero slots whose magnitudes follow the clipped gradient's
    (LARS's accumulator: times the tensor's ratio), a shadow of w plus an offset of order 1, lambda and the flag word.  The
    g = 0 tensor has lambda = 0 and a zero first moment, so that LAMB's direction is zero as well.  Computed once, never
    modified."""
    if ('in', kind) in _CACHE:
        return _CACHE[('in', kind)]
    r = np.random.RandomState(5000 + KINDS.index(kind))
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    hp = hyper(kind)
    out = []
    for i, n in enumerate(SIZES):
        el = (min(NORM[i], 100.0) if NORM[i] else 30.0) / np.sqrt(n)
        w = np.zeros(n) if i == ZERO_W else r.standard_normal(n)
        g = r.standard_normal(n) * NORM[i] / (hp['grad_scale'] * np.sqrt(n))
        lam = F32(LAMBDA[i])
        if kind == 'lars':
            W, Gh = np.sqrt((w * w).sum()), min(NORM[i], 100.0)
            ratio = hp['trust'] * W / (Gh + lam * W) if not FLAGS[i] and W > 0 and Gh > 0 else 1.0
            s0, s1 = r.standard_normal(n) * 2 * el * ratio, None
        else:
            s0, s1 = r.standard_normal(n) * 0.5 * el, (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2
            if i == ZERO_G:
                s0 = np.zeros(n)
        off = r.uniform(0.5, 1.5, n) * np.where(r.rand(n) < 0.5, -1.0, 1.0)
        out.append(dict(w=f(w), g=f(g), s0=f(s0), s1=f(s1), wd=lam, flags=FLAGS[i], shadow=None if i in NO_SHADOW else f(w + off)))
    _CACHE[('in', kind)] = out
    return out


# ---- the rule -------------------------------------------------------------------------------------------------------------
def evaluate(kind, t, hp, dtype=np.float64):
    """dict(w, g, s0, s1, ratio) of one tensor after the step, every operation in `dtype` (the norms are plain sums in it)."""
    T = dtype
    h = {k: T(v) for k, v in hp.items()}
    one, lam = T(1), T(t['wd'])
    w = t['w'].astype(T)
    g = h['grad_scale'] * t['g'].astype(T)
    norm = lambda x: np.sqrt(np.sum(x * x, dtype=T))
    G, W = norm(g), norm(w)
    c = h['clip_norm'] / max(G, h['clip_norm'])
    gh, Gh = c * g, c * G
    adapt = not (t['flags'] & NO_ADAPT)
    if kind == 'lars':
        ratio = h['trust'] * W / (Gh + lam * W) if adapt and W > 0 and Gh > 0 else one
        u = gh + lam * w
        acc = h['momentum'] * t['s0'].astype(T) + ratio * u
        return dict(w=w - h['lr'] * acc, g=gh, s0=acc, s1=None, ratio=ratio)
    m = h['beta1'] * t['s0'].astype(T) + (one - h['beta1']) * gh
    v = h['beta2'] * t['s1'].astype(T) + (one - h['beta2']) * gh * gh
    if kind == 'adamw':
        return dict(w=w - h['lr_t'] * m / (np.sqrt(v) + h['eps']) - h['lr'] * lam * w, g=gh, s0=m, s1=v, ratio=one)
    r = (m * h['bias1']) / (np.sqrt(v * h['bias2']) + h['eps']) + lam * w
    R = norm(r)
    ratio = W / R if adapt and W > 0 and R > 0 else one
    return dict(w=w - h['lr'] * ratio * r, g=r, s0=m, s1=v, ratio=ratio)


def restated(kind, t, hp, perturb=None):
    """The rule once more in fp64, with the named perturbation:
        l2_in_gradient             lambda * w is added to the scaled gradient before the norm and the clip (the old kinds' L2
                                   term) and the rule's own lambda terms are gone
        no_trust_ratio             every ratio is 1
        ratio_outside_accumulator  LARS: acc <- momentum * acc + u ; w <- w - lr * ratio * acc
        flag_ignored               NO_ADAPT is not looked at
        bias_correction_dropped    LAMB: bias1 = bias2 = 1
        w_norm_after_step          W is the norm of the w that a step with ratio 1 leaves"""
    assert perturb in (None,) + GUARDS[kind], perturb
    h = {k: np.float64(v) for k, v in hp.items()}
    one, lam = np.float64(1), np.float64(t['wd'])
    w = t['w'].astype(np.float64)
    g = h['grad_scale'] * t['g'].astype(np.float64)
    if perturb == 'l2_in_gradient':
        g, lam = g + lam * w, np.float64(0)
    if perturb == 'bias_correction_dropped':
        h['bias1'] = h['bias2'] = one
    norm = lambda x: np.sqrt(np.sum(x * x, dtype=np.float64))
    G, W = norm(g), norm(w)
    c = h['clip_norm'] / max(G, h['clip_norm'])
    gh, Gh = c * g, c * G
    adapt = perturb == 'flag_ignored' or not (t['flags'] & NO_ADAPT)
    if kind == 'lars':
        u = gh + lam * w
        if perturb == 'w_norm_after_step':
            W = norm(w - h['lr'] * (h['momentum'] * t['s0'].astype(np.float64) + u))
        ratio = h['trust'] * W / (Gh + lam * W) if adapt and W > 0 and Gh > 0 else one
        if perturb == 'no_trust_ratio':
            ratio = one
        if perturb == 'ratio_outside_accumulator':
            acc = h['momentum'] * t['s0'].astype(np.float64) + u
            return dict(w=w - h['lr'] * ratio * acc, g=gh, s0=acc, s1=None, ratio=ratio)
        acc = h['momentum'] * t['s0'].astype(np.float64) + ratio * u
        return dict(w=w - h['lr'] * acc, g=gh, s0=acc, s1=None, ratio=ratio)
    m = h['beta1'] * t['s0'].astype(np.float64) + (one - h['beta1']) * gh
    v = h['beta2'] * t['s1'].astype(np.float64) + (one - h['beta2']) * gh * gh
    if kind == 'adamw':
        return dict(w=w - h['lr_t'] * m / (np.sqrt(v) + h['eps']) - h['lr'] * lam * w, g=gh, s0=m, s1=v, ratio=one)
    r = (m * h['bias1']) / (np.sqrt(v * h['bias2']) + h['eps']) + lam * w
    R = norm(r)
    if perturb == 'w_norm_after_step':
        W = norm(w - h['lr'] * r)
    ratio = W / R if adapt and W > 0 and R > 0 else one
    if perturb == 'no_trust_ratio':
        ratio = one
    return dict(w=w - h['lr'] * ratio * r, g=r, s0=m, s1=v, ratio=ratio)


def expected(kind, perturb=None):
    """The fp64 expectation of inputs(kind) (a list of dict(w, g, s0, s1, ratio)), computed once and never modified."""
    key = ('want', kind, perturb)
    if key not in _CACHE:
        hp = hyper(kind)
        _CACHE[key] = [evaluate(kind, t, hp) if perturb is None else restated(kind, t, hp, perturb) for t in inputs(kind)]
    return _CACHE[key]


def distance(got, want, scale_from=None):
    """{output: max over the tensors of max |got - want| / max |scale|} in units of 1 (multiply TOL yourself).  The scale is
    the tensor's own max |expected| (a ratio: its own value); where that is 0 the output must be 0, and any other value is
    infinitely far."""
    worst = {}
    for a, b, s in zip(got, want, want if scale_from is None else scale_from):
        for k in OUTPUTS:
            if b[k] is None:
                assert a[k] is None, k
                continue
            err = float(np.abs(np.asarray(a[k], np.float64) - b[k]).max())
            scale = float(np.abs(s[k]).max())
            d = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
            worst[k] = max(worst.get(k, 0.0), d)
    return worst


def assert_close(got, want, what, tol=TOL, rounds=1):
    """every output of every tensor within rounds * tol of its max |expected|"""
    for i, (a, b) in enumerate(zip(got, want)):
        for k in OUTPUTS:
            if b[k] is None:
                assert a[k] is None, (what, i, k)
                continue
            err, bound = float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()), rounds * tol * float(np.abs(b[k]).max())
            assert err <= bound, '%s: %s of tensor %d: %.3e > %.3e' % (what, k, i, err, bound)


def fmt(worst):
    return ', '.join('%s %.2e' % (k, worst[k]) for k in OUTPUTS if k in worst)


# ---- running the entry point (GPU tests) ----------------------------------------------------------------------------------
def run(kind, ins, hp, shadows=True, ratio=True):
    """y3_layerwise_update_multi on fresh device copies of `ins`.  Returns (status, outputs): outputs a list of dict(w, g,
    s0, s1, ratio, shadow) of numpy arrays (ratio: None without ratio_dev; shadow: None without one)."""
    import torch
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, ctx, dev = _lib.lib(), fw.context(), fw.default_device()
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)
    ts = [dict(w=up(t['w']), g=up(t['g']), s0=up(t['s0']), s1=up(t['s1']), shadow=up(t['shadow']) if shadows else None) for t in ins]
    dp = lambda a: 0 if a is None else a.data_ptr()
    arr = (_lib.ParamDesc * len(ts))()
    for i, (t, d) in enumerate(zip(ins, ts)):
        arr[i] = _lib.ParamDesc(dp(d['w']), dp(d['g']), dp(d['s0']), dp(d['s1']), t['w'].size, t['wd'], t['flags'])
    ema = (ctypes.c_void_p * len(ts))(*[dp(d['shadow']) or None for d in ts]) if shadows else None
    rd = torch.full((len(ts),), -7.0, dtype=torch.float32, device=dev) if ratio else None
    sc = torch.empty(L.y3_layerwise_update_multi_scratch_bytes(arr, len(ts)), dtype=torch.uint8, device=dev)
    h = hp_struct(hp)
    rc = L.y3_layerwise_update_multi(ctx, KIND_ID[kind], arr, len(ts), ctypes.byref(h), ema, fw.ptr(rd), fw.ptr(sc),
                                     ctypes.c_size_t(sc.numel()))
    torch.cuda.synchronize()
    dn = lambda a: None if a is None else a.cpu().numpy()
    ratios = dn(rd)
    return rc, [dict(w=dn(d['w']), g=dn(d['g']), s0=dn(d['s0']), s1=dn(d['s1']), shadow=dn(d['shadow']),
                     ratio=None if ratios is None else ratios[i]) for i, d in enumerate(ts)]


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  The entry
# points of the layer-wise rules are added from here, as tests/ema_cases.py adds the moving average's: this module is imported
# whenever the suite is collected.  test_layerwise_update_gpu.py runs the same builder.
GUARD_SIZES = (7, 8193)                             # one element per lane, at 4-byte alignment; the second across a chunk edge


def guard_band_multi(g, kind):
    """Tensors 0 and 3 of inputs(kind) (7 and 8193 elements) in one call in a guarded arena: w, g, slots and shadows at exactly
    4-byte alignment, ratio_dev with exactly two floats, the scratch with exactly the bytes of the size function.  verify: every
    output within TOL of the fp64 rule, the shadows within the moving average's bound on the w the call produced."""
    import test_guard_bands_gpu as TG
    import ema_cases as E
    hp = hyper(kind)
    ins = [dict(t) for t in inputs(kind) if t['w'].size in GUARD_SIZES]
    assert [t['w'].size for t in ins] == list(GUARD_SIZES)
    ins[1]['shadow'] = ins[0]['shadow'][:1].repeat(GUARD_SIZES[1]) + ins[1]['w']        # (tensor 3 has none in inputs())
    want = [evaluate(kind, t, hp) for t in ins]
    arr0 = (g._lib.ParamDesc * len(ins))()
    for i, t in enumerate(ins):
        arr0[i] = g._lib.ParamDesc(None, None, None, None, t['w'].size, t['wd'], t['flags'])
    sb = g.L.y3_layerwise_update_multi_scratch_bytes(arr0, len(ins))      # (it reads the lengths only)
    specs = []
    for i, t in enumerate(ins):
        specs += [TG.INOUT('%s%d' % (k, i), t[k], align=4) for k in ('w', 'g', 's0', 's1', 'shadow') if t[k] is not None]
    specs += [TG.OUT('ratio', (len(ins),), align=4), TG.S('scratch', sb)]
    names = [s.name for s in specs]

    def call(a):
        dp = lambda k: a[k].data_ptr() if k in names else None
        arr = (g._lib.ParamDesc * len(ins))()
        for i, t in enumerate(ins):
            arr[i] = g._lib.ParamDesc(dp('w%d' % i), dp('g%d' % i), dp('s0%d' % i), dp('s1%d' % i), t['w'].size, t['wd'], t['flags'])
        ema = (ctypes.c_void_p * len(ins))(*[dp('shadow%d' % i) for i in range(len(ins))])
        h = hp_struct(hp)
        g('y3_layerwise_update_multi', g.ctx, KIND_ID[kind], arr, len(ins), ctypes.byref(h), ema, TG.P(a['ratio']),
          TG.P(a['scratch']), ctypes.c_size_t(sb))

    def verify(o):
        got = [dict(w=o['w%d' % i].numpy(), g=o['g%d' % i].numpy(), s0=o['s0%d' % i].numpy(),
                    s1=o['s1%d' % i].numpy() if 's1%d' % i in o else None, ratio=o['ratio'].numpy()[i]) for i in range(len(ins))]
        assert_close(got, want, 'guard-band %s' % kind)
        for i, t in enumerate(ins):
            r = E.worst_ratio(o['shadow%d' % i].numpy(), E.ema64(t['shadow'], got[i]['w'], hp['ema_step']),
                              E.bound(t['shadow'], got[i]['w']))
            assert r <= 1.0, (i, r)
    return TG.run_of(specs, call, names[:-1], verify)


def _register_guard_band_entries():
    import test_guard_bands_gpu as TG
    if 'y3_layerwise_update_multi_scratch_bytes' in TG.EXCLUDED:
        return
    TG.EXCLUDED['y3_layerwise_update_multi_scratch_bytes'] = 'host pointer only'
    for kind in KINDS:
        TG.entry('layerwise_update_multi-%s' % kind, ('y3_layerwise_update_multi',), guard_band_multi, kind)
    # (as in ema_cases: entries added before pytest read test_guard_bands' parametrize mark get their ids)
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entries()
