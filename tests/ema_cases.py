"""The weight moving average (include/yolo355.h, "Weight moving average") in fp64, the inputs of its kernel tests and the
derived error bound.  Shared by test_ema_cpu.py and test_ema_gpu.py; the optimizer rule itself stays the oracle's
(oracle/train_ref.py through test_optimizer_gpu).

    d_t    = min(decay, (1 + t) / (10 + t))      with warm-up, else decay
    shadow = shadow - (1 - d_t) * (shadow - w_new)
"""
import ctypes

import numpy as np

import test_optimizer_gpu as TO

EMA_SUFFIX = '/ExponentialMovingAverage'
U = 2.0 ** -24
GUARD = 100.0                  # a perturbed rule must be more than GUARD bounds away


def decay_at(decay, t, warmup=True):
    """d_t in double (TF1: ExponentialMovingAverage(decay, num_updates=t))"""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def step_at(decay, t, warmup=True):
    return 1.0 - decay_at(decay, t, warmup)


# the three step factors of the kernel tests: a plain one, 1 - 0.9998 formed in double, and the warm-up value at t = 0
EMA_STEPS = (0.1, 1.0 - 0.9998, step_at(0.9998, 0))
assert EMA_STEPS[2] == 1.0 - 1.0 / 10.0


def f32(x):
    """the value the C ABI carries: ema_step is ONE float, formed from the double"""
    return float(np.float32(x))


def ema64(shadow, w_new, ema_step):
    """The rule in fp64 on fp32 inputs, at the float the ABI carries."""
    s, w = np.asarray(shadow, np.float64), np.asarray(w_new, np.float64)
    return s - f32(ema_step) * (s - w)


def bound(shadow, w_new):
    """Element-wise gate of one update.  The kernel makes at most three fp32 roundings - the difference, the product and the
    final subtraction (an FMA only removes one).  |s - w| <= 2 max(|s|, |w|) and |ema_step| <= 1, so their sum is at most
    (2 + 2 + 1) * 2^-24 * max(|s|, |w|)."""
    return 5.0 * U * np.maximum(np.abs(np.asarray(shadow, np.float64)), np.abs(np.asarray(w_new, np.float64)))


def worst_ratio(got, want, bnd):
    """max over elements of |got - want| / bound (0 where both are 0)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max())


# ---- the kernel case: every size at which mt_update_ema_kernel can go wrong, in ONE multi-tensor call --------------------
#   1, 7     n % 4 != 0, at 4-byte alignment          4, 8192   exactly one MT_CHUNK (8192 elements)
#   8193     scalar contract across a chunk edge      8196      16-byte contract, last chunk one float4
#   16388    three chunks
# The tensor in the middle (index 4) and the last one have a NULL shadow.
SIZES = (1, 7, 4, 8192, 8196, 8193, 8196, 16388, 7)
NO_SHADOW = (4, 8)
WD = (0.0, 5e-4, 0.0, 5e-4, 5e-4, 0.0, 5e-4, 5e-4, 0.0)
NORM = (300.0, 30.0, 30.0, 300.0, 30.0, 300.0, 300.0, 300.0, 30.0)      # of grad_scale * g: above / below the clip norm of 100
SENTINEL = np.float32(-7.25)      # fills the place where a NULL-shadow tensor's shadow would lie

_CACHE = {}


def inputs(kind):
    """test_optimizer_gpu._inputs' recipe (warm, random, non-zero slots) on SIZES, plus each tensor's shadow start: w plus a
    random offset of order 1, so a kernel that leaves the shadow alone or copies w misses by many bounds.  Computed once per
    kind and never modified."""
    if kind in _CACHE:
        return _CACHE[kind]
    hp = TO.HP
    r = np.random.RandomState(3000 + TO.KINDS.index(kind))
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    out = []
    for i, n in enumerate(SIZES):
        el = min(NORM[i], hp['clip']) / np.sqrt(n)
        w = r.standard_normal(n)
        g = r.standard_normal(n) * NORM[i] / (hp['gs'] * np.sqrt(n))
        if n == 1:
            g = np.array([NORM[i] / hp['gs']])
        s0 = s1 = None
        if kind == 'momentum':
            s0 = r.standard_normal(n) * 2 * el
        elif kind == 'adam':
            s0, s1 = r.standard_normal(n) * 0.5 * el, (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2
            if n == 1:
                # Adam's step is lr_t |m| / sqrt(v): about 5e-3 from slots that follow the gradient, and a reference built with
                # the old w is then ema_step * 5e-3 = 1e-6 away at ema_step = 2e-4 - the size of the bound.  This one element
                # has a first moment far above its second (m = 1000, v = 1: a gradient that collapsed), so it moves by about
                # 3 and the old-w guard can be asserted under every step for Adam too.
                s0, s1 = np.array([1000.0]), np.array([1.0])
        elif kind == 'rmsprop':
            s0, s1 = (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2, r.standard_normal(n) * 0.01
        off = r.uniform(0.5, 1.5, n) * np.where(r.rand(n) < 0.5, -1.0, 1.0)
        out.append(dict(w=f(w), g=f(g), s0=f(s0), s1=f(s1), wd=WD[i], shadow=None if i in NO_SHADOW else f(w + off)))
    _CACHE[kind] = out
    return out


def hyper(kind):
    """the float arguments of y3_clip_update_multi(_ema) after `count`, as test_optimizer_gpu._run passes them"""
    hp, cf = TO.HP, ctypes.c_float
    lr = TO._lr_t(hp['lr'], hp['beta1'], hp['beta2'], hp['step']) if kind == 'adam' else hp['lr']
    return (cf(hp['gs']), cf(hp['clip']), cf(lr), cf(hp['momentum']), cf(hp['beta1'] if kind == 'adam' else hp['decay']),
            cf(hp['beta2']), cf(TO.EPS[kind]))


def shadow_layout():
    """Element offsets of every tensor's shadow in one flat fp32 buffer (512-byte aligned base), each at EXACTLY its contract
    alignment: 16 bytes and not 32 where n % 4 == 0, else 4 bytes and not 8.  A NULL-shadow tensor gets a place too (filled
    with SENTINEL), so its neighbours in memory are real shadows.  Returns (offsets, total elements)."""
    offs, cur = [], 0
    for n in SIZES:
        if n % 4 == 0:
            cur = (cur + 7) // 8 * 8 + 4
        else:
            cur = (cur + 1) // 2 * 2 + 1
        offs.append(cur)
        cur += n
    return offs, cur + 8


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  The three
# entry points of the moving average are added to that table from here: this module is imported whenever the suite is
# collected.  test_ema_gpu.py runs the same builders.
def guard_band_multi(g, kind, ema_step=EMA_STEPS[0]):
    """The mixed-size call in a guarded arena: shadows `inout` at exactly their contract alignment, the scratch with exactly
    the bytes of y3_clip_update_multi_ema_scratch_bytes.  verify: w, g and the slots within test_optimizer_gpu.TOL of the
    fp64 oracle, every shadow within bound() of the fp64 rule on the w the call produced."""
    import test_guard_bands_gpu as TG
    ins = inputs(kind)
    want = TO._expected(kind, ins)
    arr0 = (g._lib.ParamDesc * len(ins))()
    for i, t in enumerate(ins):
        arr0[i] = g._lib.ParamDesc(None, None, None, None, t['w'].size, t['wd'], 0)
    sb = g.L.y3_clip_update_multi_ema_scratch_bytes(arr0, len(ins))      # (it reads the lengths only)
    specs = []
    for i, t in enumerate(ins):
        al = 16 if t['w'].size % 4 == 0 else 4
        specs += [TG.INOUT('%s%d' % (k, i), t[k], align=al) for k in ('w', 'g', 's0', 's1', 'shadow') if t[k] is not None]
    specs.append(TG.S('scratch', sb))
    names = [s.name for s in specs]

    def call(a):
        dp = lambda k: a[k].data_ptr() if k in names else None
        arr = (g._lib.ParamDesc * len(ins))()
        for i, t in enumerate(ins):
            arr[i] = g._lib.ParamDesc(dp('w%d' % i), dp('g%d' % i), dp('s0%d' % i), dp('s1%d' % i), t['w'].size, t['wd'], 0)
        ema = (ctypes.c_void_p * len(ins))(*[dp('shadow%d' % i) for i in range(len(ins))])
        assert g.L.y3_clip_update_multi_ema_scratch_bytes(arr, len(ins)) == sb
        g('y3_clip_update_multi_ema', g.ctx, TO.KINDS.index(kind), arr, len(ins),
          *(hyper(kind) + (ema, ctypes.c_float(ema_step), TG.P(a['scratch']), ctypes.c_size_t(sb))))

    def verify(o):
        TG._opt_verify(o, want, ins)
        for i, t in enumerate(ins):
            if t['shadow'] is not None:
                w_new = o['w%d' % i].numpy()
                r = worst_ratio(o['shadow%d' % i].numpy(), ema64(t['shadow'], w_new, ema_step), bound(t['shadow'], w_new))
                assert r <= 1.0, (i, r)
    return TG.run_of(specs, call, names[:-1], verify)


def guard_band_single(g, n):
    """y3_ema_update on one tensor of n elements at its contract alignment"""
    import test_guard_bands_gpu as TG
    r = np.random.RandomState(4000 + n)
    w, s = r.standard_normal(n).astype(np.float32), (r.standard_normal(n) + 1.0).astype(np.float32)
    al = 16 if n % 4 == 0 else 4
    specs = [TG.INOUT('shadow', s, align=al), TG.IN('w', w, align=al)]

    def call(a):
        g('y3_ema_update', g.ctx, TG.P(a['shadow']), TG.P(a['w']), n, ctypes.c_float(EMA_STEPS[0]))

    def verify(o):
        assert worst_ratio(o['shadow'].numpy(), ema64(s, w, EMA_STEPS[0]), bound(s, w)) <= 1.0
    return TG.run_of(specs, call, ['shadow'], verify)


def _register_guard_band_entries():
    import test_guard_bands_gpu as TG
    if 'y3_clip_update_multi_ema_scratch_bytes' in TG.EXCLUDED:
        return
    TG.EXCLUDED['y3_clip_update_multi_ema_scratch_bytes'] = 'host pointer only'
    TG.entry('clip_update_multi_ema-adam', ('y3_clip_update_multi_ema',), guard_band_multi, 'adam')
    for n in (7, 8196):
        TG.entry('ema_update-n%d' % n, ('y3_ema_update',), guard_band_single, n)
    # test_guard_bands is parametrised over TABLE itself with a list of ids made when that module was imported.  When this
    # module is imported first (test_ema_cpu.py is collected before test_guard_bands_gpu.py) the new entries are in TABLE
    # before pytest reads the mark: give them their ids.  Imported later, the mark has been read already and nothing changes.
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entries()
