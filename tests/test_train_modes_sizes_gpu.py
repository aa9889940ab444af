"""The scheme of tests/test_train_sizes_gpu.py - ONE model and Trainer through changing input sizes on a poisoned workspace,
every step bit for bit against a fresh model's - with the features on that keep state of their own from one step to the next:
the SPP architecture (a 76-layer net, a materialised spp(x), an unfused BN backward under the pool), the IoU box losses
(`box_loss_key`), the layer-wise rules (a second slot, `_ratios`, the shared `opt_multi` scratch, `opt.step` in the bias
corrections), the weight moving average (the shadows, `_ema_arr`, `_ema_pending`, `averaged()` swapping tensors) and the
batch-norm exchange hook (`bn_sync_key`, the fp64 buffer).  Each has tests of its own from a fresh model at one size with the
others off; here they meet.

MODES: every new feature meets every train dtype family once.
         architecture  dtype     wgrad stream  rule   box loss  averaging          BN hook
    a    SPP           f32_wino  on            lamb   ciou      0.999, warm-up     the identity hook of test_sync_bn_step_gpu
    b    SPP           bf16      off           lars   giou      0.9, no warm-up    none
    c    default       f32       on            adamw  mse       off                the identity hook

SHAPES, in this order (data: test_train_sizes_gpu._data of the same shape, 20 classes - the detection gradient has pad lanes):
    (2,128,128)   4x4 SPP map: k = 9 and 13 coincide, k = 5 does not
    (1,160,96)    off the square, a shrink
    (3,64,64)     a batch change, inside the stale buffer
    (2,32,64)     a 1x2 SPP map: every window is the whole map; the Winograd routes step aside
    (2,256,256)   8x8: all three windows differ; stream-K and F(4x4) scratch in use
    (1,64,96)     a shrink out of the largest buffer

The fresh model of a step gets the state of just before it: every variable, opt.step, BOTH optimizer slots,
trainer.global_step (the moving average's warm-up reads it) and the shadows - handed over through Trainer.ema_assign BEFORE the
fresh Trainer's first step, so they go through `_ema_pending`, the path a checkpoint restore takes.  Compared bit for bit, and
all of it finite: the loss 5-tuple, every gradient view (lamb leaves the direction there), every variable (moving statistics
included), both slots, every shadow, trust_ratios(), and bn_sync.calls where a hook is set."""
import time

import pytest
import torch

import spp_cases as sc
import test_train_sizes_gpu as TS
from test_spp_gpu import _fresh_spp_model
from test_sync_bn_step_gpu import _sync

pytestmark = pytest.mark.gpu

CLASS_NUM, LR, WEIGHT_DECAY, BN_DECAY = TS.CLASS_NUM, TS.LR, TS.WEIGHT_DECAY, TS.BN_DECAY
SHAPES = [(2, 128, 128), (1, 160, 96), (3, 64, 64), (2, 32, 64), (2, 256, 256), (1, 64, 96)]
MODES = {
    'a': dict(spp=True, dtype='f32_wino', wgrad_stream=True, rule='lamb', box_loss='ciou', ema_decay=0.999, ema_warmup=True,
              hook=True, force=True),
    'b': dict(spp=True, dtype=TS.BF16_TRAIN, wgrad_stream=False, rule='lars', box_loss='giou', ema_decay=0.9, ema_warmup=False,
              hook=False, force=False),
    'c': dict(spp=False, dtype='f32', wgrad_stream=True, rule='adamw', box_loss='mse', ema_decay=None, ema_warmup=True,
              hook=True, force=True),
}
_PARAMS = {}


def _params(spp):
    if spp not in _PARAMS:
        _PARAMS[spp] = sc.spp_params(CLASS_NUM, seed=1) if spp else TS._params()
    return _PARAMS[spp]


def _data(shape):
    return TS._data(TS.SHAPES.index(shape))


def _new_trainer(mode, variables, state=None):
    """(model, trainer) on the current graph in `mode`, loaded with `variables`; state: what _state returned just before the
    step the new Trainer is to take"""
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    model = _fresh_spp_model(variables, CLASS_NUM, spp=mode['spp'], batch_norm_decay=BN_DECAY, weight_decay=WEIGHT_DECAY)
    model.compute_dtype = mode['dtype']
    model.box_loss = mode['box_loss']
    opt = config_optimizer(mode['rule'], LR)
    sync = False
    if mode['hook']:
        sync = _sync(lambda s, d: None)
        sync.force = mode['force']
    kw = {}
    if state is not None:
        opt.step = state['opt_step']
        opt.slots = {k: tuple(None if s is None else s.clone() for s in pair) for k, pair in state['slots'].items()}
        kw['global_step'] = state['global_step']
    trainer = training.Trainer(model, opt, wgrad_stream=mode['wgrad_stream'], sync_bn=sync, ema_decay=mode['ema_decay'],
                               ema_warmup=mode['ema_warmup'], **kw)
    if state is not None:
        for k, t in state['shadows'].items():
            trainer.ema_assign(k, t.cpu().numpy())
        assert trainer.ema is None and set(trainer._ema_pending) == set(state['shadows'])
    return model, trainer


def _state(trainer):
    """what a step starts from: every variable of scope yolov3, the optimizer's step count and both slots, the Trainer's
    global step, the shadows ({} before the first step made them: they then start as copies of the variables)"""
    import yolov3_tensorflow_amd as y3
    return dict(vars={v.op_name: v.tensor.clone() for v in y3.global_variables(scope='yolov3')},
                opt_step=trainer.opt.step, global_step=trainer.global_step,
                slots={k: tuple(None if s is None else s.clone() for s in pair) for k, pair in trainer.opt.slots.items()},
                shadows={k: t.clone() for k, t in trainer.ema_tensors().items()})


def _step(mode, model, trainer, x, yts):
    """test_train_sizes_gpu._poisoned_step, its record grown by what the modes add: both slots, the shadows, the trust ratios
    and the hook calls"""
    rec = TS._poisoned_step(model, trainer, x, yts)
    rec['slots'] = {'%s:%d' % (k, j): s.clone() for k, pair in trainer.opt.slots.items() for j, s in enumerate(pair)
                    if s is not None}
    rec['shadows'] = {k: t.clone() for k, t in trainer.ema_tensors().items()}
    ratios = trainer.trust_ratios()
    rec['ratios'] = {k: torch.tensor([v], dtype=torch.float64) for k, v in ratios.items()}
    rec['calls'] = list(trainer.bn_sync.calls) if trainer.bn_sync is not None else None
    rec['state'] = (trainer.opt.step, trainer.global_step)
    names = set(trainer.views)
    n_slots = {'lamb': 2, 'adamw': 2, 'lars': 1}[mode['rule']]
    assert set(ratios) == names and len(rec['slots']) == n_slots * len(names)
    assert set(rec['shadows']) == (names if mode['ema_decay'] else set())
    layers = model._train['topo'].layers
    bn = [i for i, l in enumerate(layers) if l['bn']]
    assert len(layers) == (76 if mode['spp'] else 75) and len(bn) == (73 if mode['spp'] else 72)
    if mode['hook']:
        assert rec['calls'] == ([(i, 0) for i in bn] + [(i, 1) for i in reversed(bn)] if mode['force'] else [])
        assert (model._train.get('bn_sync_cb') is not None) == mode['force']
    return rec


PARTS = ('views', 'vars', 'slots', 'shadows', 'ratios')


def _assert_finite(rec, what):
    TS._assert_finite(rec, what)
    for part in ('shadows', 'ratios'):
        bad = [k for k, t in rec[part].items() if not bool(torch.isfinite(t).all())]
        assert not bad, '%s: the poison reached %d of %d %s: %s' % (what, len(bad), len(rec[part]), part, bad[:6])


def _assert_same(rec, frec, what):
    TS._assert_same_bits(rec, frec, what, parts=PARTS)
    assert rec['calls'] == frec['calls'], '%s: the hook calls differ' % what
    assert rec['state'] == frec['state'], what


def _fresh_step(mode, before, x, yts):
    import yolov3_tensorflow_amd as y3
    with TS._graph({}):
        fmodel, ftrainer = _new_trainer(mode, before['vars'], before)
        with y3.variable_scope('yolov3'):
            return _step(mode, fmodel, ftrainer, x, yts)


def _both(mode, store, model, trainer, shape, what):
    """one step of the long-lived pair and the same step of a fresh one; returns the long-lived record"""
    import yolov3_tensorflow_amd as y3
    x, yts = _data(shape)
    with TS._graph(store), y3.variable_scope('yolov3'):
        before = _state(trainer)
        rec = _step(mode, model, trainer, x, yts)
    _assert_finite(rec, what)
    frec = _fresh_step(mode, before, x, yts)
    _assert_finite(frec, what + ' (fresh model)')
    _assert_same(rec, frec, what + ': long-lived against fresh')
    assert frec['ws_numel'] == frec['ws_need'] == rec['ws_need'], what
    assert rec['ws_numel'] >= rec['ws_need'], what
    return rec


@pytest.mark.parametrize('name', sorted(MODES))
def test_a_step_does_not_depend_on_the_steps_before_it_with_everything_on(name, isolated_graph):
    """MODES[name] through SHAPES by the scheme of test_train_sizes_gpu.test_a_step_does_not_depend_on_the_steps_before_it (see
    the module text for what the fresh model is handed and what is compared).  The workspace follows training._prepare's rule,
    so (3,64,64) runs inside the buffer of (2,128,128).

    After the walk of (a), on the same model and at the unchanged shape (1,64,96), two more steps: one with model.box_loss =
    'mse', then one with the hook's `force` switched off (the hook is then taken off the net, and nothing calls it).  Each is
    bit-equal to a fresh model's step with those settings: the switches move neither `ws_shape` nor a pointer, so nothing but
    the keys of their own tells the train net.

    Seconds per step are printed as test_train_sizes_gpu._long_run does.  Measured on the MI355X in one run with
    test_a_step_does_not_depend_on_the_steps_before_it[f32_wino-True-sgd] (2.7 s for its 8 shapes, 0.30 - 0.33 s a step): (b) 2.7 s
    and (c) 3.1 s for the 6 shapes, 0.35 - 0.39 s a step, the step at (2,256,256) no longer than the others, so it stays in both;
    (a) 6.8 s for its 8 steps, 0.8 s a step: the fresh Trainer takes 225 shadows through ema_assign's host copies, and the state
    handed over holds both slots and the shadows besides the variables."""
    import yolov3_tensorflow_amd as y3
    mode = dict(MODES[name])
    store, records, times = {}, [], []
    with TS._graph(store):
        model, trainer = _new_trainer(mode, _params(mode['spp']))
    cur = 0
    for i, shape in enumerate(SHAPES):
        what = 'mode %s step %d %s' % (name, i, shape)
        t0 = time.time()
        rec = _both(mode, store, model, trainer, shape, what)
        cur = max(cur, rec['ws_need'])
        assert rec['ws_numel'] == cur, what
        times.append(time.time() - t0)
        records.append(rec)
    k = SHAPES.index((3, 64, 64))
    assert max(r['ws_need'] for r in records[1:k + 1]) < records[0]['ws_need']
    assert records[k]['ws_numel'] == records[0]['ws_numel'] > records[k]['ws_need']
    assert records[-1]['state'] == (len(SHAPES), float(len(SHAPES)))
    if mode['rule'] != 'adamw':     # the kernels are adapted, gamma / beta / biases are not
        last = records[-1]['ratios']
        assert all(float(v) == 1.0 for k_, v in last.items() if not k_.endswith('/weights'))
        assert any(abs(float(v) - 1.0) > 1e-3 for k_, v in last.items() if k_.endswith('/weights'))
    if mode['ema_decay']:
        assert any(not torch.equal(records[-1]['shadows'][k_], records[-1]['vars'][k_]) for k_ in records[-1]['shadows'])
    if name == 'a':
        ptrs = lambda: {v.op_name: v.tensor.data_ptr() for v in y3.global_variables(scope='yolov3')}
        with TS._graph(store):
            p0, key0 = ptrs(), model._train['ws_shape']
        for change, field, value in (('box_loss = mse', 'box_loss', 'mse'), ('force off', 'force', False)):
            mode[field] = value
            model.box_loss = mode['box_loss']
            trainer.bn_sync.force = mode['force']
            t0 = time.time()
            rec = _both(mode, store, model, trainer, SHAPES[-1], 'mode a after the walk, %s' % change)
            times.append(time.time() - t0)
            assert rec['ws_numel'] == cur
            with TS._graph(store):
                assert ptrs() == p0 and model._train['ws_shape'] == key0
            if field == 'box_loss':     # (the mse step has a wh term, the ciou steps had none)
                assert float(rec['loss'][2]) > 0 and float(records[-1]['loss'][2]) == 0
    print('mode %s: seconds per step %s' % (name, ['%.2f' % t for t in times]))


# ---- validation inside averaged() between train steps at other sizes ------------------------------------------------------------
def _inference(variables, mode, x):
    """the inference forward of a fresh model of the mode's architecture and dtype that was ASSIGNED `variables`"""
    import yolov3_tensorflow_amd as y3
    with TS._graph({}):
        model = _fresh_spp_model(variables, CLASS_NUM, spp=mode['spp'], batch_norm_decay=BN_DECAY, weight_decay=WEIGHT_DECAY)
        model.compute_dtype = mode['dtype']
        with y3.variable_scope('yolov3'):
            return [f.clone() for f in model.forward(x, False)]


@pytest.mark.parametrize('name', ['a', 'b'])
def test_validation_inside_averaged_between_train_steps(name, isolated_graph):
    """SPP in MODES a (f32_wino) and b (bf16), one model:
        train (2,128,128) | inside averaged(): infer (1,96,160), infer (2,128,128) | train (1,160,96) | inside averaged(): infer
        (1,96,160).
    Every inference output is bit-equal to that of a fresh SPP model that was ASSIGNED the shadow values of that moment (taken
    from ema_tensors() BEFORE the context is entered) with the other variables - the moving statistics - as they are, and
    differs from the forward of the raw weights; the train step after a validation is bit-equal to a fresh model's (the
    pointer signatures of Trainer._param_descs and _vars change twice per validation); the variables' and the shadows' storage
    pointers after leaving the context are those from before."""
    import yolov3_tensorflow_amd as y3
    mode = MODES[name]
    store = {}
    with TS._graph(store):
        model, trainer = _new_trainer(mode, _params(True))

    def validate(shapes, what):
        with TS._graph(store), y3.variable_scope('yolov3'):
            raw = _state(trainer)
            variables = list(y3.global_variables(scope='yolov3'))
            ptrs = [v.tensor.data_ptr() for v in variables], {k: t.data_ptr() for k, t in trainer.ema_tensors().items()}
            assert len(raw['shadows']) == len(trainer.views) == 225
            averaged = dict(raw['vars'])
            averaged.update(raw['shadows'])
            assert any(not torch.equal(averaged[k], raw['vars'][k]) for k in raw['shadows'])
            outs = []
            with trainer.averaged():
                for shape in shapes:
                    outs.append([f.clone() for f in model.forward(_data(shape)[0], False)])
                with pytest.raises(RuntimeError):
                    trainer.step(*_data(shapes[0]))
            assert ptrs == ([v.tensor.data_ptr() for v in variables], {k: t.data_ptr() for k, t in trainer.ema_tensors().items()})
            after = _state(trainer)
            for part in ('vars', 'shadows'):
                assert all(torch.equal(after[part][k], raw[part][k]) for k in raw[part]), part
        for shape, got in zip(shapes, outs):
            x = _data(shape)[0]
            assert TS._all_finite(got), (what, shape)
            want, plain = _inference(averaged, mode, x), _inference(raw['vars'], mode, x)
            for k, (g, r, p) in enumerate(zip(got, want, plain)):
                assert g.shape == r.shape and torch.equal(g, r), \
                    '%s %s %s: feature map %d differs from a fresh model\'s on the shadows' % (name, what, shape, k + 1)
                assert not torch.equal(g, p), '%s %s %s: feature map %d is the raw weights\'' % (name, what, shape, k + 1)
        return outs

    first = _both(mode, store, model, trainer, (2, 128, 128), 'mode %s first step' % name)
    assert first['state'] == (1, 1.0)
    out1 = validate([(1, 96, 160), (2, 128, 128)], 'after one step')
    _both(mode, store, model, trainer, (1, 160, 96), 'mode %s: the train step after a validation' % name)
    out2 = validate([(1, 96, 160)], 'after two steps')
    assert not any(torch.equal(a, b) for a, b in zip(out1[0], out2[0])), 'the second step changed no averaged output'
