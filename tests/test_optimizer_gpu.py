"""The optimizer update rules WITH STATE against the fp64 rule (oracle/train_ref.py: clip_by_norm, apply_update; ref:
train.py:112-115, utils/misc_utils.py:151-161, TF1 definitions).

Part A: the two kernels (y3_clip_update, y3_clip_update_multi) from warm, random, non-zero slots.
Part B: training.Trainer.apply_gradients over three rounds with a callable learning-rate schedule, chained on the CPU.

Both parts end with sensitivity guards that run NO broken kernel: references with one rule perturbed are built on the CPU
and must lie more than 100 tolerances away from what the GPU produced (GUARDS_A, GUARDS_B name them)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS, blob_images

KINDS = ('sgd', 'momentum', 'adam', 'rmsprop')
TOL = 2e-6                     # of each output tensor's max |expected|
GUARD = 100.0                  # a perturbed rule must be more than GUARD tolerances away

# ---- part A: inputs ------------------------------------------------------------------------------------------------
# 7, 255: n % 4 != 0 (scalar path of mt_prepare_kernel); 8192: exactly one MT_CHUNK; 8196: vector path, last chunk of one
# float4; 8193: scalar path across a chunk edge; 300000: > 512 x 256, grad_prepare_kernel strides; 18, 1024.
SIZES = (7, 255, 8192, 8196, 8193, 300000, 18, 1024)
WD = (0.0, 5e-4, 5e-4, 0.0, 5e-4, 5e-4, 0.0, 0.0)
NORM = (300.0, 30.0, 30.0, 300.0, 300.0, 300.0, 30.0, 30.0)      # of grad_scale * g: above / below the clip norm of 100
EPS_TENSOR, EPS_SLICE = 7, slice(256, 512)                        # where eps is comparable to what stands under the root (wd = 0)
# The C ABI carries the hyper-parameters as floats, so the rule is evaluated at the float32 values of 0.8 / 0.9 / 0.999: the
# kernels form (1 - beta) in fp32, and 1 - float32(0.999) is 1.3e-5 (relative) away from 0.001 (1 - float32(0.9): 3.6e-7 from
# 0.1).  That is TF's fp32 kernel too, and no rounding error of the kernels: an expectation built from the exact decimals
# puts it on a slot that starts from zero (adam's v after round 1 of part B was 1.29e-5 of its max off such an expectation,
# measured), and hides it behind beta * slot when the slot is warm.
F32 = lambda x: float(np.float32(x))
HP = dict(gs=0.5, clip=100.0, lr=5e-2, momentum=F32(0.8), decay=F32(0.9), beta1=F32(0.9), beta2=F32(0.999), step=3)
EPS = dict(sgd=0.0, momentum=0.0, adam=1e-8, rmsprop=1e-10)
# which perturbed rule each kind's test would catch (part A)
GUARDS_A = dict(sgd=('no_weight_decay',),
                momentum=('no_weight_decay', 'momentum_is_decay'),
                adam=('no_weight_decay', 'betas_swapped', 'eps_inside_root'),
                rmsprop=('no_weight_decay', 'eps_outside_root', 'momentum_zero', 'momentum_is_decay'))


def _inputs(kind):
    """One list of tensors per kind (numpy float32): w, g, slot0, slot1.  Slots start from random non-zero state: momentum
    accumulator and adam m signed, adam v and rmsprop ms positive, rmsprop mom small and signed; their magnitudes follow the
    clipped gradient's, so that every step is O(lr)."""
    r = np.random.RandomState(1000 + KINDS.index(kind))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    out = []
    for i, n in enumerate(SIZES):
        el = min(NORM[i], HP['clip']) / np.sqrt(n)             # size of an element of the clipped gradient
        w = r.standard_normal(n)
        g = r.standard_normal(n) * NORM[i] / (HP['gs'] * np.sqrt(n))
        s0 = s1 = None
        if kind == 'momentum':
            s0 = r.standard_normal(n) * 2 * el
        elif kind == 'adam':
            s0 = r.standard_normal(n) * 0.5 * el
            s1 = (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2
        elif kind == 'rmsprop':
            s0 = (el * (0.5 + np.abs(r.standard_normal(n)))) ** 2
            s1 = r.standard_normal(n) * 0.01
        if i == EPS_TENSOR:
            m = EPS_SLICE.stop - EPS_SLICE.start
            sign = np.where(r.rand(m) < 0.5, -1.0, 1.0)
            if kind == 'adam':                                  # sqrt(v) ~ 1e-8 = eps; |m| / (sqrt(v) + eps) ~ 0.25: a sane step
                g[EPS_SLICE] = r.standard_normal(m) * 2e-10
                s0[EPS_SLICE] = sign * r.uniform(2e-9, 8e-9, m)
                s1[EPS_SLICE] = 1e-16 * r.uniform(0.5, 2.0, m)
            elif kind == 'rmsprop':                             # ms ~ 1e-10 = eps; lr * g / sqrt(ms + eps) ~ 7e-3
                g[EPS_SLICE] = sign * r.uniform(2e-6, 6e-6, m)
                s0[EPS_SLICE] = 1e-10 * r.uniform(0.5, 2.0, m)
        out.append(dict(w=f(w), g=f(g), s0=None if s0 is None else f(s0), s1=None if s1 is None else f(s1), wd=WD[i]))
    return out


def _lr_t(lr, beta1, beta2, step):
    return lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)


# ---- the rule in fp64, and its perturbed forms -------------------------------------------------------------------------
def _update64(kind, w, g, s0, s1, lr, step, eps, hp, perturb=None):
    """(new w, new slot0, new slot1) in fp64 from the clipped gradient g.  perturb=None goes through the oracle
    (train_ref.apply_update); the perturbed forms restate the rule with ONE thing changed (and `_own_rule_is_the_oracles`
    checks that the restatement without a change is the oracle's, bit for bit)."""
    from oracle import train_ref
    if perturb is None:
        slots = {}
        if kind == 'momentum':
            slots = dict(accum=s0.clone())
        elif kind == 'adam':
            slots = dict(m=s0.clone(), v=s1.clone())
        elif kind == 'rmsprop':
            slots = dict(ms=s0.clone(), mom=s1.clone())
        new = train_ref.apply_update(kind, w, g, slots, lr=lr, step=step, momentum=hp['momentum'], decay=hp['decay'],
                                     beta1=hp['beta1'], beta2=hp['beta2'], eps=eps if kind in ('adam', 'rmsprop') else None)
        order = dict(sgd=(), momentum=('accum',), adam=('m', 'v'), rmsprop=('ms', 'mom'))[kind]
        got = [slots[k] for k in order] + [None, None]
        return new, got[0], got[1]
    return _own_rule(kind, w, g, s0, s1, lr, step, eps, hp, perturb)


def _own_rule(kind, w, g, s0, s1, lr, step, eps, hp, perturb):
    momentum, decay, beta1, beta2 = hp['momentum'], hp['decay'], hp['beta1'], hp['beta2']
    if perturb == 'momentum_is_decay':
        momentum, decay = decay, momentum
    if perturb == 'momentum_zero':
        momentum = 0.0
    if kind == 'sgd':
        return w - lr * g, None, None
    if kind == 'momentum':
        a = s0 * momentum + g
        return w - lr * a, a, None
    if kind == 'adam':
        lr_t = _lr_t(lr, beta1, beta2, step)                    # (the step size keeps its betas: only the slot updates swap)
        if perturb == 'betas_swapped':
            beta1, beta2 = beta2, beta1
        m = s0 * beta1 + (1 - beta1) * g
        v = s1 * beta2 + (1 - beta2) * g * g
        den = torch.sqrt(v + eps) if perturb == 'eps_inside_root' else torch.sqrt(v) + eps
        return w - lr_t * m / den, m, v
    ms = s0 * decay + (1 - decay) * g * g
    den = torch.sqrt(ms) + eps if perturb == 'eps_outside_root' else torch.sqrt(ms + eps)
    mom = s1 * momentum + lr * g / den
    return w - mom, ms, mom


def _expected(kind, inputs, perturb=None, hp=HP):
    """fp64: g <- grad_scale*g + wd*w, clip_by_norm, update.  Returns a list of dict(w, g, s0, s1) of float64 arrays."""
    from oracle import train_ref
    t64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
    out = []
    for t in inputs:
        w, g, s0, s1 = t64(t['w']), t64(t['g']), t64(t['s0']), t64(t['s1'])
        wd = 0.0 if perturb == 'no_weight_decay' else t['wd']
        gc = train_ref.clip_by_norm(g * hp['gs'] + wd * w, hp['clip'])
        p = None if perturb == 'no_weight_decay' else perturb
        nw, n0, n1 = _update64(kind, w, gc, s0, s1, hp['lr'], hp['step'], EPS[kind], hp, p)
        out.append(dict(w=nw.numpy(), g=gc.numpy(), s0=None if n0 is None else n0.numpy(),
                        s1=None if n1 is None else n1.numpy()))
    return out


_CACHE = {}


def _case(kind):
    """The inputs and the fp64 expectation of a kind, computed once and shared by both entry points (never modified)."""
    if kind not in _CACHE:
        inputs = _inputs(kind)
        _CACHE[kind] = (inputs, _expected(kind, inputs))
    return _CACHE[kind]


def _distance(got, want, scale_from, keys):
    """max over tensors and keys of max|got - want| / max|scale_from|: in units of 1 (multiply TOL yourself)"""
    worst = {}
    for a, b, s in zip(got, want, scale_from):
        for k in keys:
            if b[k] is None:
                continue
            d = float(np.abs(np.asarray(a[k], np.float64) - b[k]).max() / np.abs(s[k]).max())
            worst[k] = max(worst.get(k, 0.0), d)
    return worst


# ---- the two entry points ------------------------------------------------------------------------------------------------
def _run(kind, entry, inputs, hp=HP):
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, ctx, dev = _lib.lib(), fw.context(), fw.default_device()
    k = KINDS.index(kind)
    lr = _lr_t(hp['lr'], hp['beta1'], hp['beta2'], hp['step']) if kind == 'adam' else hp['lr']
    decay = hp['beta1'] if kind == 'adam' else hp['decay']
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)
    ts = [dict(w=up(t['w']), g=up(t['g']), s0=up(t['s0']), s1=up(t['s1']), wd=t['wd']) for t in inputs]
    cf = ctypes.c_float
    if entry == 'multi':
        arr = (_lib.ParamDesc * len(ts))()
        dp = lambda a: 0 if a is None else a.data_ptr()
        for i, t in enumerate(ts):
            arr[i] = _lib.ParamDesc(dp(t['w']), dp(t['g']), dp(t['s0']), dp(t['s1']), t['w'].numel(), t['wd'], 0)
        sc = torch.empty(L.y3_clip_update_multi_scratch_bytes(arr, len(ts)), dtype=torch.uint8, device=dev)
        _lib.check(L.y3_clip_update_multi(ctx, k, arr, len(ts), cf(hp['gs']), cf(hp['clip']), cf(lr), cf(hp['momentum']),
                                          cf(decay), cf(hp['beta2']), cf(EPS[kind]), fw.ptr(sc), ctypes.c_size_t(sc.numel())))
    else:
        sc = torch.empty(L.y3_optimizer_scratch_bytes(), dtype=torch.uint8, device=dev)
        for t in ts:
            _lib.check(L.y3_clip_update(ctx, k, fw.ptr(t['w']), fw.ptr(t['g']), fw.ptr(t['s0']), fw.ptr(t['s1']),
                                        t['w'].numel(), cf(t['wd']), cf(hp['gs']), cf(hp['clip']), cf(lr), cf(hp['momentum']),
                                        cf(decay), cf(hp['beta2']), cf(EPS[kind]), fw.ptr(sc)))
    torch.cuda.synchronize()
    dn = lambda a: None if a is None else a.cpu().numpy()
    return [dict(w=dn(t['w']), g=dn(t['g']), s0=dn(t['s0']), s1=dn(t['s1'])) for t in ts]


def test_own_rule_is_the_oracles():
    """The restated rule that the perturbed references are built from IS the oracle's when nothing is perturbed (bit for
    bit, fp64): a guard then differs from the expectation by the named perturbation alone.  (fp64 on the CPU: no GPU.)"""
    for kind in KINDS:
        inputs, want = _case(kind)
        t64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
        for t, e in zip(inputs, want):
            nw, n0, n1 = _own_rule(kind, t64(t['w']), torch.tensor(e['g']), t64(t['s0']), t64(t['s1']), HP['lr'], HP['step'],
                                   EPS[kind], HP, None)
            np.testing.assert_array_equal(nw.numpy(), e['w'])
            for a, b in ((n0, e['s0']), (n1, e['s1'])):
                assert (a is None) == (b is None)
                if a is not None:
                    np.testing.assert_array_equal(a.numpy(), b)


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['single', 'multi'])
@pytest.mark.parametrize('kind', KINDS)
def test_optimizer_kernels_match_the_fp64_rule_from_warm_slots(kind, entry):
    """y3_clip_update / y3_clip_update_multi from non-zero slots, grad_scale 0.5, weight decay on some tensors, some tensors
    clipped, lr 5e-2, momentum 0.8 / decay = beta1 0.9 / beta2 0.999 (as float32), against train_ref.clip_by_norm + apply_update in fp64.
    w, the clipped g left in place and both slots: each within 2e-6 of the tensor's max |expected|.

    Worst error over the tensors, as a fraction of the tensor's max: a CPU fp32 evaluation of the oracle at the exact
    decimals / the kernels on the MI355X (the larger of the two entry points; they differ only in adam's g, 1.1e-7 single):
        kind       w                  g                  slot 0             slot 1
        sgd        4.8e-8 / 3.9e-8    1.1e-7 / 9.4e-8    -                  -
        momentum   4.9e-8 / 9.4e-8    1.1e-7 / 9.9e-8    1.3e-7 / 8.8e-8    -
        adam       5.4e-8 / 4.8e-8    1.1e-7 / 1.3e-7    9.7e-8 / 7.4e-8    8.8e-8 / 8.0e-8
        rmsprop    4.9e-8 / 5.0e-8    1.1e-7 / 1.0e-7    2.2e-7 / 8.2e-8    1.3e-7 / 1.6e-7
    (the test prints them).  The hyper-parameters are the float32 values the C ABI carries (see HP).

    Guards (GUARDS_A; no broken kernel runs): the fp64 rule with weight decay dropped, beta1 and beta2 swapped in adam's slot
    updates, adam's eps inside the root, rmsprop's eps outside it, rmsprop's momentum 0, momentum and decay exchanged - each
    must be more than 100 tolerances from the GPU's result on w or a slot.  The one exception is dropped weight decay for
    sgd, which is looked for on the clipped g: sgd has no slot, and on w it is lr*wd*w = 2.5e-5 |w|, below 100 tolerances by
    construction.  With a slot it must show there (fp64 against fp64, in tolerances: momentum's accumulator 369, adam's m
    157, rmsprop's mom 1128)."""
    inputs, want = _case(kind)
    got = _run(kind, entry, inputs)
    worst = _distance(got, want, want, ('w', 'g', 's0', 's1'))
    print('optimizer %s/%s: worst error / max|expected|: %s' % (
        kind, entry, ', '.join('%s %.2e' % (k, worst[k]) for k in ('w', 'g', 's0', 's1') if k in worst)))
    for i, (a, b) in enumerate(zip(got, want)):
        for key in ('w', 'g', 's0', 's1'):
            if b[key] is None:
                assert a[key] is None
                continue
            err, bound = float(np.abs(a[key].astype(np.float64) - b[key]).max()), TOL * float(np.abs(b[key]).max())
            assert err <= bound, '%s of tensor %d (%d elements): %.3e > %.3e' % (key, i, SIZES[i], err, bound)
    # clipping happened where it should
    for i, a in enumerate(got):
        norm = float(np.sqrt((a['g'].astype(np.float64) ** 2).sum()))
        assert abs(norm - 100.0) < 1e-2 if NORM[i] > 100.0 else norm < 99.0, (i, norm)
    for perturb in GUARDS_A[kind]:
        keys = ('w', 'g') if (perturb, kind) == ('no_weight_decay', 'sgd') else ('w', 's0', 's1')
        d = _distance(got, _expected(kind, inputs, perturb), want, keys)
        assert max(d.values()) > GUARD * TOL, '%s would pass: %s' % (perturb, d)


# ---- part B: Trainer.apply_gradients over three rounds ---------------------------------------------------------------
_HEAD = lambda j: 'yolov3/yolov3_head/Conv_%d/' % j
SCHEDULE = lambda s: 1e-2 * 0.5 ** s
ROUND_SCALE = (0.01, 1.0, 0.01)          # of a standard-normal gradient: in round 2 the kernels (>= 32768 elements) clip
OPT_HP = dict(momentum=HP['momentum'], decay=HP['decay'], beta1=HP['beta1'], beta2=HP['beta2'])     # (float32 values: see HP)
WEIGHT_DECAY = 5e-4
# which perturbed chain each kind's test would catch (part B)
GUARDS_B = dict(sgd=('constant_lr', 'wd_on_every_tensor'),
                momentum=('constant_lr', 'wd_on_every_tensor', 'slots_forgotten'),
                adam=('constant_lr', 'wd_on_every_tensor', 'slots_forgotten', 'adam_step_stays_1'),
                rmsprop=('constant_lr', 'wd_on_every_tensor', 'slots_forgotten'))


def _chain(kind, start, grads, perturb=None):
    """The reference over the rounds, fp64: apply_update(kind, w, clip_by_norm(g + wd*w), slots, lr=schedule(step-1),
    step=step), wd on the names ending in /weights, slots from empty (rmsprop's ms from ones).  Returns, per round,
    {name: dict(w, g, s0, s1)}."""
    from oracle import train_ref
    w = {k: torch.tensor(v, dtype=torch.float64) for k, v in start.items()}
    slots = {k: {} for k in start}
    order = dict(sgd=(), momentum=('accum',), adam=('m', 'v'), rmsprop=('ms', 'mom'))[kind]
    rounds = []
    for step, gr in enumerate(grads, 1):
        rec = {}
        for k in start:
            wd = WEIGHT_DECAY if k.endswith('/weights') or perturb == 'wd_on_every_tensor' else 0.0
            g = train_ref.clip_by_norm(torch.tensor(gr[k], dtype=torch.float64) + wd * w[k], 100.0)
            if perturb == 'slots_forgotten':
                slots[k] = {}
            lr = SCHEDULE(0 if perturb == 'constant_lr' else step - 1)
            w[k] = train_ref.apply_update(kind, w[k], g, slots[k], lr=lr, step=1 if perturb == 'adam_step_stays_1' else step,
                                          **OPT_HP)
            s = [slots[k][n].numpy().copy() for n in order] + [None, None]
            rec[k] = dict(w=w[k].numpy().copy(), g=g.numpy(), s0=s[0], s1=s[1])
        rounds.append(rec)
    return rounds


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_apply_gradients_over_three_rounds_matches_the_chained_fp64_rule(kind, isolated_graph):
    """training.Trainer.apply_gradients three times, with a CALLABLE schedule (1e-2 * 0.5**global_step) and update_vars = the
    last three head convs (kernels, BN gamma / beta, the detection bias), on seeded random gradients written into
    trainer.flat (round 2 scaled so that the kernels clip).  After each round the variables, the clipped gradients
    (trainer.views) and the slots (trainer.opt.slots) are held to the chained fp64 rule: 2e-6 of the tensor's max in round 1,
    k times that in round k (the fp32 state carries forward).  Variables outside update_vars keep every bit; global_step
    advances by 3.  Measured on the MI355X, worst error / (round * max|expected|): sgd 5.3e-8, momentum 4.9e-8, adam 1.2e-7,
    rmsprop 1.3e-7 (printed).

    Guards (GUARDS_B), each a chain on the CPU that must end more than 100 tolerances from the GPU's state on some tensor:
    the schedule read at global_step 0 every round, weight decay on gamma / beta / bias too, slots that do not persist, and
    for adam lr_t computed with t = 1 every round."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from oracle import yolo_ref, train_ref
    params = yolo_ref.synthetic_params(80, seed=1)
    y3.reset_default_graph()
    model = y3.yolov3(80, COCO_ANCHORS, batch_norm_decay=0.99, weight_decay=WEIGHT_DECAY)
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    for v in y3.global_variables(scope='yolov3'):
        v.assign(params[v.op_name])
    prefixes = tuple(_HEAD(j) for j in (20, 21, 22))
    upd = [v for v in y3.global_variables(scope='yolov3') if v.op_name.startswith(prefixes) and v.trainable]
    names = sorted(v.op_name for v in upd)
    assert len(names) == 8 and sum(n.endswith('/weights') for n in names) == 3 and sum(n.endswith('/biases') for n in names) == 1
    trainer = training.Trainer(model, training.Optimizer(kind, SCHEDULE, **OPT_HP), update_vars=upd)
    x = blob_images(11, 1, 64)
    yts = train_ref.synthetic_targets(12, 1, [64, 64], 80, COCO_ANCHORS, max_boxes=3)
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, is_training=True)
        training.compute_loss(model, fms, yts)
        trainer.backward()                                       # allocates trainer.flat / views
    assert sorted(trainer.views) == names
    torch.cuda.synchronize()
    by_name = {v.op_name: v for v in y3.global_variables(scope='yolov3')}
    before = {k: v.tensor.clone() for k, v in by_name.items()}  # (after the training forward: it moves the BN statistics)
    start = {k: before[k].cpu().numpy() for k in names}
    for k in names:
        np.testing.assert_array_equal(start[k], params[k])
    step0 = trainer.global_step
    rng = np.random.RandomState(77 + KINDS.index(kind))
    grads, got = [], []
    for scale in ROUND_SCALE:
        flat = (rng.standard_normal(trainer.flat.numel()) * scale).astype(np.float32)
        grads.append({k: flat[trainer.offsets[k]:trainer.offsets[k] + start[k].size].reshape(start[k].shape) for k in names})
        trainer.flat.copy_(torch.from_numpy(flat))
        with y3.variable_scope('yolov3'):
            trainer.apply_gradients()
        torch.cuda.synchronize()
        rec = {}
        for k in names:
            s0, s1 = trainer.opt.slots[k]
            rec[k] = dict(w=by_name[k].numpy().copy(), g=trainer.views[k].cpu().numpy(),
                          s0=None if s0 is None else s0.cpu().numpy(), s1=None if s1 is None else s1.cpu().numpy())
        got.append(rec)
    want = _chain(kind, start, grads)
    worst = 0.0
    for rnd, (a, b) in enumerate(zip(got, want), 1):
        for k in names:
            for key in ('w', 'g', 's0', 's1'):
                if b[k][key] is None:
                    assert a[k][key] is None
                    continue
                err, scale = float(np.abs(a[k][key].astype(np.float64) - b[k][key]).max()), float(np.abs(b[k][key]).max())
                worst = max(worst, err / scale / rnd)
                assert err <= rnd * TOL * scale, 'round %d, %s of %s: %.3e > %.3e' % (rnd, key, k, err, rnd * TOL * scale)
    print('apply_gradients %s: worst error / (round * max|expected|) = %.2e' % (kind, worst))
    # round 2 clipped the kernels and nothing else
    for k in names:
        assert (np.sqrt((want[1][k]['g'] ** 2).sum()) > 99.0) == k.endswith('/weights'), k
    # nothing outside update_vars moved, and the step counters did
    for k, v in by_name.items():
        if k not in trainer.views:
            assert torch.equal(v.tensor, before[k]), k
    assert trainer.global_step == step0 + 3 and trainer.opt.step == 3
    # guards
    last = len(ROUND_SCALE)
    for perturb in GUARDS_B[kind]:
        other = _chain(kind, start, grads, perturb)[-1]
        far = max(float(np.abs(got[-1][k][key].astype(np.float64) - other[k][key]).max() / np.abs(want[-1][k][key]).max())
                  for k in names for key in ('w', 'g', 's0', 's1') if other[k][key] is not None)
        assert far > GUARD * last * TOL, '%s would pass: %.3e' % (perturb, far)
