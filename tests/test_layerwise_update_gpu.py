"""y3_layerwise_update_multi (AdamW, LARS, LAMB; include/yolo355.h, "Layer-wise update rules") against the fp64 rule of
tests/layerwise_cases.py, and training.Trainer.apply_gradients over three rounds with those kinds.

Tolerance: test_optimizer_gpu.TOL = 2e-6 of each output tensor's max |expected| (a tensor's ratio: of its own value).  A float32
numpy evaluation of the rules on the same inputs is 0.7e-7 to 1.6e-7 away from fp64 (test_layerwise_update_cpu.py prints and
gates it at TOL / 8), so no output needs a wider gate.  The perturbed forms of layerwise_cases.GUARDS are 78,000 to 1e9
tolerances from the rule on their most sensitive output (fp64 against fp64, printed there); no broken kernel runs."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS, blob_images
import ema_cases as E
import layerwise_cases as LC

pytestmark = pytest.mark.gpu
_GPU = {}


def _result(kind, shadows):
    """the entry on the shared inputs, run once per (kind, shadows) and never modified"""
    if (kind, shadows) not in _GPU:
        rc, got = LC.run(kind, LC.inputs(kind), LC.hyper(kind), shadows=shadows)
        assert rc == 0
        _GPU[(kind, shadows)] = got
    return _GPU[(kind, shadows)]


def _same_bits(a, b, keys=('w', 'g', 's0', 's1', 'ratio', 'shadow')):
    for i, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert (x[k] is None) == (y[k] is None), (i, k)
            if x[k] is not None:
                assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), 'tensor %d: %s differs' % (i, k)


@pytest.mark.parametrize('shadows', [False, True], ids=['plain', 'shadows'])
@pytest.mark.parametrize('kind', LC.KINDS)
def test_entry_matches_the_fp64_rule(kind, shadows):
    """w, g as left in place (the clipped gradient; LAMB: the direction r), both slots and ratio_dev of ten tensors in one call
    - warm slots, grad_scale 0.5, lambda 0 and 5e-2, two NO_ADAPT tensors, a zero w and a zero g, tensors above and below the
    clip norm - each within 2e-6 of its max |expected|.

    Worst error over the tensors as a fraction of the tensor's max, float32 numpy / the kernels on the MI355X (printed):
        kind     w                  g                  slot 0             slot 1             ratio
        adamw    1.5e-7 / 1.5e-7    8.6e-8 / 8.6e-8    7.3e-8 / 7.3e-8    7.3e-8 / 7.3e-8    0 / 0
        lars     7.1e-8 / 7.1e-8    9.8e-8 / 9.8e-8    1.1e-7 / 1.1e-7    -                  8.0e-8 / 8.0e-8
        lamb     9.9e-8 / 9.9e-8    1.6e-7 / 1.6e-7    9.2e-8 / 9.2e-8    9.6e-8 / 9.6e-8    7.1e-8 / 9.7e-8
    (the element-wise arithmetic is compiled without contraction, so it rounds as numpy's does; the norms are summed in
    another order and show in LAMB's ratio alone.)"""
    want, got = LC.expected(kind), _result(kind, shadows)
    print('layerwise %s%s: worst error / max|expected|: %s' % (kind, ' + shadows' if shadows else '', LC.fmt(LC.distance(got, want))))
    LC.assert_close(got, want, kind)
    for i, (t, a, e) in enumerate(zip(LC.inputs(kind), got, want)):
        assert (a['ratio'] == 1.0) == (kind == 'adamw' or bool(t['flags']) or i in (LC.ZERO_W, LC.ZERO_G)), (i, a['ratio'])
        if kind != 'lamb':      # clipping happened where it should
            norm = float(np.sqrt((a['g'].astype(np.float64) ** 2).sum()))
            assert abs(norm - 100.0) < 1e-2 if LC.NORM[i] > 100.0 else norm < 80.0, (i, norm)


@pytest.mark.parametrize('kind', LC.KINDS)
def test_shadows_change_no_bit_of_the_step_and_follow_the_moving_average_rule(kind):
    """The call with shadows and the call without: w, g, slots and ratios bit for bit the same.  Every shadow within the
    moving-average block's bound (5 * 2^-24 * max(|s|, |w_new|)) of the fp64 rule on the w the call stored; the tensor with a
    NULL entry has none.  A call without ratio_dev gives the same bits too."""
    plain, with_sh = _result(kind, False), _result(kind, True)
    _same_bits(plain, with_sh, keys=('w', 'g', 's0', 's1', 'ratio'))
    hp = LC.hyper(kind)
    worst = 0.0
    for i, (t, o) in enumerate(zip(LC.inputs(kind), with_sh)):
        if t['shadow'] is None:
            assert o['shadow'] is None and i in LC.NO_SHADOW
            continue
        assert not np.array_equal(o['shadow'], t['shadow'])
        worst = max(worst, E.worst_ratio(o['shadow'], E.ema64(t['shadow'], o['w'], hp['ema_step']), E.bound(t['shadow'], o['w'])))
    print('layerwise %s: worst shadow error / bound = %.3f' % (kind, worst))
    assert worst <= 1.0
    rc, no_ratio = LC.run(kind, LC.inputs(kind), hp, shadows=True, ratio=False)
    assert rc == 0
    _same_bits(with_sh, no_ratio, keys=('w', 'g', 's0', 's1', 'shadow'))


@pytest.mark.parametrize('kind', LC.KINDS)
def test_two_calls_give_the_same_bits(kind):
    rc, again = LC.run(kind, LC.inputs(kind), LC.hyper(kind), shadows=True)
    assert rc == 0
    _same_bits(_result(kind, True), again)


@pytest.mark.parametrize('kind', LC.KINDS)
def test_every_perturbed_rule_is_far_from_what_the_kernels_computed(kind):
    """layerwise_cases.GUARDS: the rule with the L2 term in the gradient, without the ratio, with LARS's ratio outside the
    accumulator, with NO_ADAPT ignored, without LAMB's bias corrections, with W taken after the step - each more than 100
    tolerances from the GPU's result on some output.  References only: no broken kernel runs."""
    got, want = _result(kind, False), LC.expected(kind)
    for perturb in LC.GUARDS[kind]:
        d = LC.distance(got, LC.expected(kind, perturb), scale_from=want)
        assert max(d.values()) > LC.GUARD * LC.TOL, '%s would pass: %s' % (perturb, d)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _small(kind):
    """two tensors, 8 elements (the 16-byte contract) and 7"""
    r = np.random.RandomState(6000)
    mk = lambda n: r.standard_normal(n).astype(np.float32)
    return [dict(w=mk(n), g=mk(n), s0=mk(n), s1=np.abs(mk(n)) if LC.SLOTS[kind] == 2 else None, shadow=mk(n), wd=LC.F32(5e-2),
                 flags=0) for n in (8, 7)]


def _call(kind, kind_id=None, hp=None, hp_null=False, drop=(), shift=None, alias=None, wd=None, scratch=None, ema_null=False,
          unchanged=True):
    """One call on _small(kind) with ONE thing wrong.  Every tensor lies 16 bytes into a buffer of its own (`shift`: another
    number of floats); alias: {tensor: key} makes that tensor's shadow pointer the pointer of its w / g / slot.  Returns the
    status; unchanged: asserts that no bit of any buffer, the bytes around the tensors included, nor ratio_dev changed."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, ctx, dev = _lib.lib(), fw.context(), fw.default_device()
    ins, shift, alias, wd = _small(kind), shift or {}, alias or {}, wd or {}
    bufs, ptr = {}, {}
    for i, t in enumerate(ins):
        for k in ('w', 'g', 's0', 's1', 'shadow'):
            if t[k] is None:
                continue
            off = shift.get((i, k), 4)
            b = torch.zeros(t[k].size + 8, dtype=torch.float32, device=dev)
            b[off:off + t[k].size].copy_(torch.from_numpy(t[k]))
            bufs[(i, k)], ptr[(i, k)] = b, b.data_ptr() + 4 * off
    before = {key: b.clone() for key, b in bufs.items()}
    arr = (_lib.ParamDesc * len(ins))()
    p = lambda i, k: None if (i, k) in drop else ptr.get((i, k))
    for i, t in enumerate(ins):
        arr[i] = _lib.ParamDesc(p(i, 'w'), p(i, 'g'), p(i, 's0'), p(i, 's1'), t['w'].size, wd.get(i, t['wd']), t['flags'])
    ema = (ctypes.c_void_p * len(ins))(*[ptr[(i, alias[i])] if i in alias else ptr[(i, 'shadow')] for i in range(len(ins))])
    nb = L.y3_layerwise_update_multi_scratch_bytes(arr, len(ins))
    sc = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
    sp, sn = sc.data_ptr(), nb
    if scratch == 'small':
        sn = nb - 1
    elif scratch == 'misaligned':
        sp += 4
    elif scratch == 'null':
        sp = None
    rd = torch.zeros(len(ins), dtype=torch.float32, device=dev)
    h = LC.hp_struct(dict(LC.hyper(kind), **(hp or {})))
    rc = L.y3_layerwise_update_multi(ctx, LC.KIND_ID[kind] if kind_id is None else kind_id, arr, len(ins),
                                     None if hp_null else ctypes.byref(h), None if ema_null else ema, fw.ptr(rd),
                                     None if sp is None else ctypes.c_void_p(sp), ctypes.c_size_t(sn))
    torch.cuda.synchronize()
    if unchanged:
        for key, b in bufs.items():
            assert torch.equal(b.view(torch.int32), before[key].view(torch.int32)), key
        assert not rd.any()
    return rc


def _refusals(kind):
    cases = [('kind 3', dict(kind_id=3)), ('kind 7', dict(kind_id=7)), ('kind -1', dict(kind_id=-1)), ('NULL hp', dict(hp_null=True)),
             ('slot0 missing', dict(drop={(1, 's0')})), ('w missing', dict(drop={(0, 'w')})), ('NULL scratch', dict(scratch='null'))]
    if LC.SLOTS[kind] == 2:
        cases.append(('slot1 missing', dict(drop={(0, 's1')})))
    for f in LC.HP_FIELDS:
        cases.append(('%s NaN' % f, dict(hp={f: float('nan')})))
    cases += [('lr inf', dict(hp=dict(lr=float('inf')))), ('clip -inf', dict(hp=dict(clip_norm=float('-inf')))),
              ('lambda NaN', dict(wd={1: float('nan')})), ('lambda inf', dict(wd={0: float('inf')}))]
    cases += [('negative %s' % f, dict(hp={f: -1e-3})) for f in ('trust', 'lr', 'eps')]
    cases += [('negative lambda', dict(wd={1: -5e-2})), ('ema_step -0.1', dict(hp=dict(ema_step=-0.1))),
              ('ema_step 1.5', dict(hp=dict(ema_step=1.5))), ('ema_step -0.1, no shadows', dict(hp=dict(ema_step=-0.1), ema_null=True))]
    keys = ('w', 'g', 's0', 'shadow') + (('s1',) if LC.SLOTS[kind] == 2 else ())
    cases += [('misaligned %s' % k, dict(shift={(0, k): 1})) for k in keys]                 # n % 4 == 0 at 4 bytes
    cases += [('shadow is %s' % k, dict(alias={i: k})) for k in keys[:3] + keys[4:] for i in (0, 1)]
    cases += [('scratch too small', dict(scratch='small')), ('scratch misaligned', dict(scratch='misaligned'))]
    return cases


@pytest.mark.parametrize('kind', LC.KINDS)
def test_refusals_leave_every_tensor_unchanged(kind):
    """Y3_EINVAL before any launch, with w, g, slots, shadows and ratio_dev bit-unchanged: a kind outside 4..6, a NULL hp, w,
    slot or scratch, each member of hp NaN, an infinite lr or clip, a non-finite or negative lambda, a negative trust, lr or
    eps, ema_step outside [0, 1] (with and without shadows), w, g, a slot or a shadow of an 8-element tensor at 4-byte
    alignment, a shadow that is its tensor's w, g or slot, a scratch one byte short or misaligned.  The same call with
    nothing wrong succeeds (so no case is refused for another reason)."""
    from yolov3_tensorflow_amd import _lib
    from yolov3_tensorflow_amd import framework as fw
    for name, mut in _refusals(kind):
        assert _call(kind, **mut) == _lib.Y3_EINVAL, name
    assert len(_lib.lib().y3_last_error()) > 0
    fw.check_context()
    # nothing wrong: accepted, with the 7-element tensors at 4-byte alignment
    assert _call(kind, shift={(1, k): 1 for k in ('w', 'g', 's0', 's1', 'shadow')}, unchanged=False) == 0


@pytest.mark.parametrize('kind', LC.KINDS)
def test_old_entries_refuse_the_new_kinds(kind):
    """y3_clip_update, y3_clip_update_multi and y3_clip_update_multi_ema go on taking kinds 0..3 only."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, ctx, dev = _lib.lib(), fw.context(), fw.default_device()
    k, cf = LC.KIND_ID[kind], ctypes.c_float
    ts = [torch.full((8,), 0.5 + i, dtype=torch.float32, device=dev) for i in range(5)]       # w, g, slot0, slot1, shadow
    before = [t.clone() for t in ts]
    arr = (_lib.ParamDesc * 1)(_lib.ParamDesc(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), 8, 0.0, 0))
    hp = (cf(1.0), cf(100.0), cf(1e-2), cf(0.9), cf(0.9), cf(0.999), cf(1e-8))
    sc = torch.zeros(max(L.y3_clip_update_multi_ema_scratch_bytes(arr, 1), L.y3_optimizer_scratch_bytes()), dtype=torch.uint8, device=dev)
    ema = (ctypes.c_void_p * 1)(ts[4].data_ptr())
    assert L.y3_clip_update_multi(ctx, k, arr, 1, *(hp + (fw.ptr(sc), ctypes.c_size_t(sc.numel())))) == _lib.Y3_EINVAL
    assert L.y3_clip_update_multi_ema(ctx, k, arr, 1, *(hp + (ema, cf(0.1), fw.ptr(sc), ctypes.c_size_t(sc.numel())))) == _lib.Y3_EINVAL
    assert L.y3_clip_update(ctx, k, fw.ptr(ts[0]), fw.ptr(ts[1]), fw.ptr(ts[2]), fw.ptr(ts[3]), 8, cf(0.0), *(hp + (fw.ptr(sc),))) == _lib.Y3_EINVAL
    torch.cuda.synchronize()
    for a, b in zip(ts, before):
        assert torch.equal(a, b)
    # and they still take kind 3 with the same arguments
    assert L.y3_clip_update_multi(ctx, 3, arr, 1, *(hp + (fw.ptr(sc), ctypes.c_size_t(sc.numel())))) == 0
    torch.cuda.synchronize()
    assert not torch.equal(ts[0], before[0])


@pytest.mark.parametrize('kind', LC.KINDS)
def test_guard_bands_at_7_and_8193_elements(kind):
    """layerwise_cases.guard_band_multi through tests/guarded.py: tensors of 7 and 8193 elements (one element per lane, the
    second across a chunk edge) with slots, shadows, ratio_dev and the scratch at exactly their sizes and 4-byte alignment
    between poisoned bands.  No guard byte changes, the 0xFF and the 0x7F pass agree bit for bit, the outputs pass the gates."""
    import guarded
    import test_guard_bands_gpu as TG
    g = TG.G()
    run = LC.guard_band_multi(g, kind)
    arena = guarded.build(g.dev, run.specs)
    kept = guarded.run_passes(arena, lambda: run.call(arena), run.outputs, sync=torch.cuda.synchronize)
    g.fw.check_context()
    assert g.called == {'y3_layerwise_update_multi'}
    guarded.assert_passes_identical(kept, 'layerwise-%s' % kind)
    run.verify(kept[0])


# ---- Trainer.apply_gradients over three rounds ----------------------------------------------------------------------------
_HEAD = lambda j: 'yolov3/yolov3_head/Conv_%d/' % j
SCHEDULE = lambda s: 1e-2 * 0.5 ** s
ROUND_SCALE = (0.01, 1.0, 0.01)          # of a standard-normal gradient: in round 2 the kernels (>= 32768 elements) clip
OPT_HP = dict(momentum=LC.F32(0.8), beta1=LC.F32(0.9), beta2=LC.F32(0.999), trust=LC.F32(0.02))
WEIGHT_DECAY = 5e-2
EMA_DECAY = 0.9
GUARDS_B = dict(adamw=('constant_lr', 'lambda_on_every_tensor', 'slots_forgotten', 'step_stays_1'),
                lars=('constant_lr', 'lambda_on_every_tensor', 'slots_forgotten', 'every_tensor_adapted'),
                lamb=('constant_lr', 'lambda_on_every_tensor', 'slots_forgotten', 'step_stays_1', 'every_tensor_adapted'))


def _chain(kind, start, grads, eps, perturb=None):
    """The fp64 rule over the rounds: lr = schedule(step - 1), the bias corrections of step t, lambda and the adaptation on the
    names ending in /weights, slots from zeros.  Returns, per round, {name: dict(w, g, s0, s1, ratio)}."""
    w = {k: np.asarray(v, np.float64) for k, v in start.items()}
    slots = {k: [np.zeros_like(w[k]) if j < LC.SLOTS[kind] else None for j in range(2)] for k in start}
    rounds = []
    for step, gr in enumerate(grads, 1):
        hp = LC.hyper(kind, step=1 if perturb == 'step_stays_1' else step, grad_scale=1.0, eps=eps, ema_step=0.0,
                      lr=SCHEDULE(0 if perturb == 'constant_lr' else step - 1), **OPT_HP)
        rec = {}
        for k in start:
            kernel = k.endswith('/weights')
            if perturb == 'slots_forgotten':
                slots[k] = [None if s is None else np.zeros_like(s) for s in slots[k]]
            t = dict(w=w[k], g=gr[k], s0=slots[k][0], s1=slots[k][1],
                     wd=LC.F32(WEIGHT_DECAY) if kernel or perturb == 'lambda_on_every_tensor' else 0.0,
                     flags=0 if kernel or perturb == 'every_tensor_adapted' else LC.NO_ADAPT)
            rec[k] = LC.evaluate(kind, t, hp)
            w[k], slots[k] = rec[k]['w'], [rec[k]['s0'], rec[k]['s1']]
        rounds.append(rec)
    return rounds


@pytest.mark.parametrize('kind', LC.KINDS)
def test_apply_gradients_over_three_rounds_matches_the_chained_fp64_rule(kind, isolated_graph, tmp_path):
    """training.Trainer.apply_gradients three times with a CALLABLE schedule (1e-2 * 0.5**global_step), weight_decay 5e-2,
    trust 0.02, a weight moving average (ema_decay 0.9) and update_vars = the last three head convs (kernels, BN gamma /
    beta, the detection bias), on seeded random gradients written into trainer.flat (round 2 scaled so that the kernels clip).
    After each round the variables, trainer.views (the clipped gradient; lamb: the direction), the slots and trust_ratios() are
    held to the chained fp64 rule: 2e-6 of the tensor's max in round 1, k times that in round k.  gamma, beta and the bias
    report ratio 1 exactly; every shadow is within the moving average's bound of the rule on the w the step stored; variables
    outside update_vars keep every bit.  Measured on the MI355X, worst error / (round * max|expected|): adamw 8.4e-8, lars
    1.5e-7, lamb 3.2e-7; the shadows at most 0.43 of their bound (printed).

    Between rounds 2 and 3 the state is saved (Saver: slots under the new names, optimizer/step, global_step, the averages);
    after round 3 it is restored into a NEW Optimizer and round 3 runs again: every variable, slot, gradient view, ratio and
    shadow is bit for bit what the uninterrupted round 3 left.

    Guards (GUARDS_B), each a chain on the CPU that must end more than 100 tolerances from the GPU's state: the schedule read
    at global_step 0 every round, lambda on gamma / beta / bias too, slots that do not persist, the bias corrections of t = 1
    every round, and gamma / beta / bias adapted like kernels."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils import misc_utils
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
    assert len(names) == 8 and sum(n.endswith('/weights') for n in names) == 3
    make_opt = lambda: training.Optimizer(kind, SCHEDULE, **OPT_HP)
    trainer = training.Trainer(model, make_opt(), update_vars=upd, ema_decay=EMA_DECAY)
    eps = trainer.opt.epsilon
    assert eps == dict(adamw=1e-8, lars=1e-10, lamb=1e-6)[kind]
    x = blob_images(11, 1, 64)
    yts = train_ref.synthetic_targets(12, 1, [64, 64], 80, COCO_ANCHORS, max_boxes=3)
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, is_training=True)
        training.compute_loss(model, fms, yts)
        trainer.backward()                                       # allocates trainer.flat / views / the shadows
    assert sorted(trainer.views) == names
    torch.cuda.synchronize()
    by_name = {v.op_name: v for v in y3.global_variables(scope='yolov3')}
    before = {k: v.tensor.clone() for k, v in by_name.items()}
    start = {k: before[k].cpu().numpy() for k in names}
    step0 = trainer.global_step
    rng = np.random.RandomState(177 + LC.KINDS.index(kind))

    def snapshot():
        torch.cuda.synchronize()
        ratios = trainer.trust_ratios()
        rec = {}
        for k in names:
            s0, s1 = trainer.opt.slots[k]
            rec[k] = dict(w=by_name[k].numpy().copy(), g=trainer.views[k].cpu().numpy(), s0=s0.cpu().numpy(),
                          s1=None if s1 is None else s1.cpu().numpy(), ratio=np.float64(ratios[k]),
                          shadow=trainer.ema_tensors()[k].cpu().numpy())
        return rec

    def one_round(flat):
        trainer.flat.copy_(torch.from_numpy(flat))
        with y3.variable_scope('yolov3'):
            trainer.apply_gradients()
        return snapshot()

    grads, flats, got, path = [], [], [], None
    worst_shadow = 0.0
    for rnd, scale in enumerate(ROUND_SCALE, 1):
        flat = (rng.standard_normal(trainer.flat.numel()) * scale).astype(np.float32)
        flats.append(flat)
        grads.append({k: flat[trainer.offsets[k]:trainer.offsets[k] + start[k].size].reshape(start[k].shape) for k in names})
        if rnd == 3:
            path = misc_utils.Saver(upd).save(str(tmp_path / 'round2'), optimizer=trainer.opt, global_step=trainer.global_step,
                                              averages=trainer)
        shadows = {k: t.cpu().numpy() for k, t in trainer.ema_tensors().items()}
        ema_step = trainer.ema_step_at(trainer.global_step)
        got.append(one_round(flat))
        for k in names:
            w_new = got[-1][k]['w']
            worst_shadow = max(worst_shadow, E.worst_ratio(got[-1][k]['shadow'], E.ema64(shadows[k], w_new, ema_step),
                                                           E.bound(shadows[k], w_new)))
    assert worst_shadow <= 1.0, worst_shadow
    want = _chain(kind, start, grads, eps)
    worst = 0.0
    for rnd, (a, b) in enumerate(zip(got, want), 1):
        LC.assert_close([a[k] for k in names], [b[k] for k in names], 'round %d' % rnd, rounds=rnd)
        worst = max(worst, max(LC.distance([a[k] for k in names], [b[k] for k in names]).values()) / rnd)
        for k in names:
            if not k.endswith('/weights') or kind == 'adamw':
                assert a[k]['ratio'] == 1.0, k
            else:
                assert abs(a[k]['ratio'] - 1.0) > 0.2, (k, a[k]['ratio'])
    print('apply_gradients %s: worst error / (round * max|expected|) = %.2e, shadows %.3f of their bound' % (kind, worst, worst_shadow))
    for k in names:     # round 2 clipped the kernels and nothing else (lamb leaves the direction in g: look at the chain's G)
        g2 = np.asarray(grads[1][k], np.float64)
        assert (np.sqrt((g2 * g2).sum()) > 100.0) == k.endswith('/weights'), k
    for k, v in by_name.items():
        if k not in trainer.views:
            assert torch.equal(v.tensor, before[k]), k
    assert trainer.global_step == step0 + 3 and trainer.opt.step == 3
    # the keys of the checkpoint, then round 3 again from it
    stored = np.load(path)
    for k in names:
        for s in misc_utils._SLOT_NAMES[kind]:
            assert k + '/' + s in stored.files
    fresh = make_opt()
    trainer.opt = fresh
    trainer.global_step = misc_utils.Saver(upd).restore(path, optimizer=fresh, averages=trainer)
    assert trainer.global_step == step0 + 2 and fresh.step == 2
    again = one_round(flats[2])
    _same_bits([got[2][k] for k in names], [again[k] for k in names])
    # guards
    last = len(ROUND_SCALE)
    for perturb in GUARDS_B[kind]:
        other = _chain(kind, start, grads, eps, perturb)[-1]
        d = LC.distance([got[-1][k] for k in names], [other[k] for k in names], scale_from=[want[-1][k] for k in names])
        assert max(d.values()) > LC.GUARD * last * LC.TOL, '%s would pass: %s' % (perturb, d)
