"""The train step across changing input sizes, on a poisoned workspace (the reference trains multi-scale: a new input
size every ten batches, train.py, and evaluates between epochs in the same process).

What survives from one train step to the next - the workspace and its `ws_shape` key, the library's y3_train_state, the
inference plan cache, the folded inference parameters, the scratch buffers that only grow - has otherwise only been tested
with the next step at the same shape.  Here ONE model and Trainer walk through SHAPES, and every step is compared BIT FOR
BIT with the same step taken by a fresh model that was loaded with the variables of that moment.  Before every step, of
either model, the whole train workspace is filled with 0xFF bytes (a NaN in fp32 and in bf16) and the flat gradient buffer
with NaN: a kernel that reads a workspace byte nothing wrote in THIS step turns a result into NaN, or at least into other
bits than the fresh model's.  (What the poison cannot show: a block the step's own arena freed and handed out again holds
THIS step's values - finite, and the same in both models.  Without the memset of the loss gradients their pad lanes go
unnoticed up to (2,128,128), where they land in such a block, and turn 210 of 222 gradients into NaN at (2,256,256).)

SHAPES is the smallest set found that holds every kind of change: a grow, a shrink into a larger stale buffer, an h / w
swap at equal pixel count, a batch change, a 32-pixel side (its /32 map is one pixel wide: the Winograd routes refuse it
and the direct kernel takes over mid-run), the return to the first shape - and two shapes from reading the route
functions (y3_route_train_fwd / y3_route_dgrad / y3_route_wgrad, csrc/y3_abi.hip):
  (2,256,256)  the smallest shape at which both (a) a 3x3 conv takes the stream-K schedule (use_streamk: >= 32 tiles of 128 rows
               x 128 channels; the 64->128 convs on the 64x64 map have 64, at (2,128,128) no conv has more than 16) and (b)
               'f32_wino' prefers the F(4x4,3x3) kernel (y3_conv_wino44_preferred: >= 128 blocks of 16 tiles x 64 channels;
               the 32->64 conv on the 128x128 map has exactly 128).  Both use the step's scratch (`sk_ws`).
  (1,64,96)    a shrink again, out of the buffer the largest shape left.
The Winograd weight gradient's own threshold (y3_conv_wgrad_wino_eligible: 8 / tile columns + 1 tile rows must fit the
map) is crossed inside SHAPES as it is (the 4x4 and 3x5 maps are refused, the 8x8 and 6x10 ones taken).  The F(4x4,3x3)
DATA gradient and the two-kernel form need 2,048 tiles on the /4 map or Cout >= 512 with 128 blocks (n * h * w >= 2 * 512
* 512): left to the tests that run those shapes at one size; the image-range split starts at 2^29 elements
(test_large_tensors_gpu.py)."""
import contextlib
import time

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
from test_train_gpu import _blob_images_hw, _fresh_model

pytestmark = pytest.mark.gpu

CLASS_NUM = 20          # 75 detection channels, gradient rows padded to 96: pad lanes exist
LR, WEIGHT_DECAY, BN_DECAY = 1e-3, 5e-4, 0.99      # test_train_gpu._step_matches_oracle
SEQUENCE = [(2, 128, 128), (1, 160, 96), (1, 96, 160), (3, 64, 64), (2, 32, 64), (2, 128, 128)]
SHAPES = SEQUENCE + [(2, 256, 256), (1, 64, 96)]
BF16_TRAIN = 'bf16'     # the train dtype of test_train_bf16_gpu.py; also the bf16 inference dtype

_DATA = {}              # step index -> (images, [y_true_13, _26, _52]) on the device
_PARAMS = {}
_LONG_RUNS = {}         # (dtype, wgrad_stream, optimizer) -> the long-lived run's records (shared between tests 1 and 2)
_ORACLE = {}            # step index -> fp64 / fp32 training forward of the oracle


def _params():
    if not _PARAMS:
        from oracle import yolo_ref
        _PARAMS.update(yolo_ref.synthetic_params(CLASS_NUM, seed=1))
    return _PARAMS


def _targets(seed, n, h, w):
    """y_true of the three scales ([n, h/s, w/s, 3, 5 + C + 1], utils/data_utils.py:51-115) with one or two boxes per image
    ON EVERY SCALE, whatever the image size: a cell, an anchor slot, a centre inside the cell, the slot's anchor scaled by
    U(0.6, 1.4) and clipped to the image, a class, a mix-up weight from U(0.2, 1) in the last channel (1 elsewhere)."""
    rng = np.random.RandomState([seed, n, h, w])
    out = []
    for si, s in enumerate((32, 16, 8)):
        gh, gw = h // s, w // s
        y = np.zeros((n, gh, gw, 3, 6 + CLASS_NUM), np.float32)
        y[..., -1] = 1.0
        for i in range(n):
            cells = rng.permutation(gh * gw)[:min(2, gh * gw)]
            for c in cells:
                gy, gx, k = int(c) // gw, int(c) % gw, rng.randint(3)
                aw, ah = COCO_ANCHORS[3 * (2 - si) + k] * rng.uniform(0.6, 1.4)
                y[i, gy, gx, k, 0:2] = ((gx + rng.uniform(0.1, 0.9)) * s, (gy + rng.uniform(0.1, 0.9)) * s)
                y[i, gy, gx, k, 2:4] = (min(aw, w - 2.0), min(ah, h - 2.0))
                y[i, gy, gx, k, 4] = 1.0
                y[i, gy, gx, k, 5 + rng.randint(CLASS_NUM)] = 1.0
                y[i, gy, gx, k, -1] = rng.uniform(0.2, 1.0)
        out.append(y)
    return out


def _data(i):
    if i not in _DATA:
        from yolov3_tensorflow_amd import framework as fw
        n, h, w = SHAPES[i]
        _DATA[i] = (fw.as_device_f32(_blob_images_hw(40 + i, n, h, w)),
                    [fw.as_device_f32(y) for y in _targets(60 + i, n, h, w)])
    return _DATA[i]


@contextlib.contextmanager
def _graph(store):
    """The variables of `store` (a dict, filled by the block where it creates some) as the default graph for the block:
    a long-lived model and the fresh ones each keep variables of the same names."""
    from yolov3_tensorflow_amd import framework as fw
    saved = dict(fw._VARIABLES)
    fw._VARIABLES.clear()
    fw._VARIABLES.update(store)
    fw._bump_global_version()
    try:
        yield
    finally:
        store.clear()
        store.update(fw._VARIABLES)
        fw._VARIABLES.clear()
        fw._VARIABLES.update(saved)
        fw._bump_global_version()


def _new_trainer(params, dtype, wgrad_stream, optimizer='sgd', opt_state=None):
    """(model, trainer) on the current graph, loaded with `params`; opt_state: (step count, {op_name: momentum slot})"""
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    model = _fresh_model(params, CLASS_NUM, batch_norm_decay=BN_DECAY, weight_decay=WEIGHT_DECAY)
    model.compute_dtype = dtype
    opt = config_optimizer(optimizer, LR)
    if opt_state is not None:
        opt.step = opt_state[0]
        opt.slots = {k: (s.clone(), None) for k, s in opt_state[1].items()}
    return model, training.Trainer(model, opt, wgrad_stream=wgrad_stream)


def _snapshot(trainer):
    """every variable of scope yolov3 (moving statistics included), the optimizer's step count and momentum slots"""
    import yolov3_tensorflow_amd as y3
    variables = {v.op_name: v.tensor.clone() for v in y3.global_variables(scope='yolov3')}
    slots = {k: s[0].clone() for k, s in trainer.opt.slots.items() if s[0] is not None}
    return variables, (trainer.opt.step, slots)


def _poisoned_step(model, trainer, x, yts):
    """One trainer.step whose workspace (sized for this shape by training._prepare, as the step itself would) is full of
    0xFF bytes and whose gradient buffer is full of NaN.  Under the model's graph and variable scope.  Returns the step's
    record: loss 5-tuple, gradient views, variables, momentum slots, and the workspace's size / what this shape needs."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training, _lib, framework as fw
    # the second-stream setting the step is about to install (Trainer.step): _prepare re-keys the workspace on it
    model.wgrad_stream = trainer._calib['step'] < 4 if trainer._calib is not None else trainer.wgrad_choice
    st, net, layer_vars = training._prepare(model, x)
    n, h, w, _ = x.shape
    need = _lib.lib().y3_net_train_workspace_bytes(net, st['vars_all'], n, h, w)
    ws = st['ws']
    ws.fill_(0xFF)
    trainer._alloc_grads(layer_vars, x.device)
    # Trainer: backward writes every trainable view (test_partial_update_vars_on_the_second_stream_change_no_bit starts
    # from NaN too); the pads between views (gradient_layout aligns to 16 bytes) are read by nothing on one rank
    trainer.flat.fill_(float('nan'))
    loss = trainer.step(x, yts)
    assert model._train['ws'] is ws, 'the step did not run in the workspace that was poisoned'
    fw.check_context()
    variables, (_, slots) = _snapshot(trainer)
    assert set(trainer.views) == set(v.op_name for v in y3.global_variables(scope='yolov3') if v.trainable)
    return dict(loss=torch.stack(loss).cpu(), views={k: v.clone() for k, v in trainer.views.items()}, vars=variables,
                slots=slots, ws_numel=ws.numel(), ws_need=int(need))


def _all_finite(tensors):
    return bool(torch.stack([torch.isfinite(t).all() for t in tensors]).all())


def _assert_finite(rec, what):
    assert bool(torch.isfinite(rec['loss']).all()), '%s: loss %s' % (what, rec['loss'].tolist())
    for part in ('views', 'vars', 'slots'):
        if rec[part] and not _all_finite(list(rec[part].values())):
            bad = [k for k, t in rec[part].items() if not bool(torch.isfinite(t).all())]
            raise AssertionError('%s: the poison reached %d of %d %s: %s' % (what, len(bad), len(rec[part]), part, bad[:6]))


def _assert_same_bits(a, b, what, parts=('views', 'vars', 'slots')):
    assert a['loss'].view(torch.int32).tolist() == b['loss'].view(torch.int32).tolist(), \
        '%s: loss %s against %s' % (what, a['loss'].tolist(), b['loss'].tolist())
    for part in parts:
        assert set(a[part]) == set(b[part]), '%s: %s' % (what, part)
        diff = [k for k in a[part] if not torch.equal(a[part][k], b[part][k])]
        assert not diff, '%s: %d of %d %s differ in some bit: %s' % (what, len(diff), len(a[part]), part, diff[:6])


def _long_run(dtype, wgrad_stream, optimizer='sgd', against_fresh=True):
    """The long-lived model and Trainer through SHAPES; every step also taken by a fresh model (against_fresh) and held to
    it bit for bit.  Returns the long-lived run's records."""
    import yolov3_tensorflow_amd as y3
    key = (dtype, wgrad_stream, optimizer)
    if key in _LONG_RUNS and not against_fresh:
        return _LONG_RUNS[key]
    store, records, times = {}, [], []
    with _graph(store):
        model, trainer = _new_trainer(_params(), dtype, wgrad_stream, optimizer)
    cur = 0
    for i, shape in enumerate(SHAPES):
        x, yts = _data(i)
        what = '%s wgrad_stream=%s %s step %d %s' % (dtype, wgrad_stream, optimizer, i, shape)
        t0 = time.time()
        with _graph(store), y3.variable_scope('yolov3'):
            before = _snapshot(trainer)
            rec = _poisoned_step(model, trainer, x, yts)
        _assert_finite(rec, what)
        # training._prepare keeps the workspace whenever it is large enough, and replaces it by exactly what is needed
        cur = rec['ws_need'] if cur < rec['ws_need'] else cur
        assert rec['ws_numel'] == cur, what
        if against_fresh:
            fresh_store = {}
            with _graph(fresh_store):
                fmodel, ftrainer = _new_trainer(before[0], dtype, wgrad_stream, optimizer, before[1])
                with y3.variable_scope('yolov3'):
                    frec = _poisoned_step(fmodel, ftrainer, x, yts)
            _assert_finite(frec, what + ' (fresh model)')
            _assert_same_bits(rec, frec, what + ': long-lived against fresh')
            assert frec['ws_numel'] == frec['ws_need'] == rec['ws_need']
            del fmodel, ftrainer, frec, fresh_store
        times.append(time.time() - t0)
        records.append(rec)
    # the shrink ran inside the stale buffer of the first shape
    k = SHAPES.index((3, 64, 64))
    assert max(r['ws_need'] for r in records[1:k + 1]) < records[0]['ws_need']
    assert records[k]['ws_numel'] == records[0]['ws_numel'] > records[k]['ws_need']
    print('%s wgrad_stream=%s %s: seconds per step %s' % (dtype, wgrad_stream, optimizer, ['%.2f' % t for t in times]))
    if optimizer == 'sgd':
        assert not records[0]['slots']
    if key == ('f32', False, 'sgd'):      # (the one run test_auto_calibration_under_changing_sizes compares with)
        _LONG_RUNS[key] = records
    return records


@pytest.mark.parametrize('dtype,wgrad_stream,optimizer', [
    ('f32', False, 'sgd'), ('f32', True, 'sgd'), ('f32_wino', True, 'sgd'), ('f32_bf16x6', False, 'sgd'),
    (BF16_TRAIN, False, 'sgd'), (BF16_TRAIN, True, 'sgd'),
    # warm momentum slots, handed to the fresh model through Optimizer.slots
    ('f32', True, 'momentum')])
def test_a_step_does_not_depend_on_the_steps_before_it(dtype, wgrad_stream, optimizer, isolated_graph):
    """One model and Trainer through SHAPES; before each step the workspace is 0xFF and the gradient buffer NaN.  Each step
    against a fresh model (a new graph, a new Trainer, a new workspace, poisoned alike) loaded with the variables, the
    optimizer's step count and the momentum slots of just before: the loss 5-tuple, every gradient view of the flat
    buffer, every variable (moving means and variances included) and every slot equal bit for bit, and all of it finite.
    The workspace follows training._prepare's rule (kept while large enough), so the step at (3,64,64) runs inside the
    buffer of (2,128,128)."""
    records = _long_run(dtype, wgrad_stream, optimizer)
    assert len(records) == len(SHAPES)
    if optimizer == 'momentum':
        assert records[-1]['slots'] and any(bool(s.abs().max() > 0) for s in records[-1]['slots'].values())


def test_auto_calibration_under_changing_sizes(isolated_graph):
    """Trainer(wgrad_stream='auto') over the eight SHAPES: second stream on for steps 0-3, off from step 4 - the (2,32,64)
    step, a shrink, where _train_net also drops `ws_shape` - and its choice after step 6.  Workspace and gradient buffer
    poisoned as above.  Every step bit-equal to the wgrad_stream=False run of the same scheme on the same data (which
    test_a_step_does_not_depend_on_the_steps_before_it holds to fresh models); which stream wins is a timing."""
    import yolov3_tensorflow_amd as y3
    assert len(SHAPES) == 8 and SHAPES[4] == (2, 32, 64)
    want = _long_run('f32', False, 'sgd', against_fresh=False)
    store = {}
    with _graph(store):
        model, trainer = _new_trainer(_params(), 'f32', 'auto')
    assert trainer.wgrad_choice is None
    for i, shape in enumerate(SHAPES):
        x, yts = _data(i)
        with _graph(store), y3.variable_scope('yolov3'):
            rec = _poisoned_step(model, trainer, x, yts)
        assert model.wgrad_stream == (i < 4 if i < 7 else trainer.wgrad_choice)
        what = "wgrad_stream='auto' step %d %s" % (i, shape)
        _assert_finite(rec, what)
        _assert_same_bits(rec, want[i], what + ': against the one-stream run')
        if i < 6:
            assert trainer.wgrad_choice is None and not hasattr(trainer, 'wgrad_calibration')
    assert set(trainer.wgrad_calibration) == {'ms_with', 'ms_without'}
    assert all(np.isfinite(v) and v > 0 for v in trainer.wgrad_calibration.values())
    assert isinstance(trainer.wgrad_choice, bool)


def _fresh_inference(variables, dtype, x):
    import yolov3_tensorflow_amd as y3
    with _graph({}):
        model = _fresh_model(variables, CLASS_NUM, batch_norm_decay=BN_DECAY, weight_decay=WEIGHT_DECAY)
        model.compute_dtype = dtype
        with y3.variable_scope('yolov3'):
            return [f.clone() for f in model.forward(x, False)]


@pytest.mark.parametrize('dtype', ['f32', 'f32_wino', BF16_TRAIN])
def test_validation_forwards_between_train_steps(dtype, isolated_graph):
    """train (2,128,128) | infer (1,96,160) | infer (2,128,128) | train (1,160,96) | infer (1,96,160), one model: every
    inference output bit-equal to that of a fresh model loaded with the variables of that moment (the plan cache at
    another size, the moving statistics re-folded and the weights re-packed after a step), the second train step bit-equal
    to a fresh model's (the train state after inference forwards).
    Then forward(is_training=True) at (2,128,128) | infer (1,96,160): after a step, Trainer.apply_gradients touches every
    updated variable and yolov3._get_net re-folds ALL layers when any version moved, so the step's own touch() of the moving
    statistics cannot be told apart there; a training forward moves the moving statistics and nothing else."""
    import yolov3_tensorflow_amd as y3
    store = {}
    with _graph(store):
        model, trainer = _new_trainer(_params(), dtype, True)
    ia, ib, ic = SHAPES.index((2, 128, 128)), SHAPES.index((1, 96, 160)), SHAPES.index((1, 160, 96))

    def infer(i, what):
        x = _data(i)[0]
        with _graph(store), y3.variable_scope('yolov3'):
            got = [f.clone() for f in model.forward(x, False)]
            variables = _snapshot(trainer)[0]
        want = _fresh_inference(variables, dtype, x)
        assert _all_finite(got), what
        for k, (g, r) in enumerate(zip(got, want)):
            assert g.shape == r.shape and torch.equal(g, r), '%s %s: feature map %d differs from a fresh model\'s' % (dtype, what, k + 1)
        return got

    with _graph(store), y3.variable_scope('yolov3'):
        first = _poisoned_step(model, trainer, *_data(ia))
    _assert_finite(first, 'first step')
    fb = infer(ib, 'after one step, at (1,96,160)')
    infer(ia, 'after one step, at (2,128,128)')
    with _graph(store), y3.variable_scope('yolov3'):
        before = _snapshot(trainer)
        rec = _poisoned_step(model, trainer, *_data(ic))
    with _graph({}):
        fmodel, ftrainer = _new_trainer(before[0], dtype, True, 'sgd', before[1])
        with y3.variable_scope('yolov3'):
            frec = _poisoned_step(fmodel, ftrainer, *_data(ic))
    _assert_finite(rec, 'second step')
    _assert_same_bits(rec, frec, '%s: the train step after two inference forwards against a fresh model\'s' % dtype)
    fb2 = infer(ib, 'after two steps, at (1,96,160)')
    assert not any(torch.equal(a, b) for a, b in zip(fb, fb2)), 'the second step changed no inference output'
    # the moving statistics alone: a training forward moves nothing else, and the next inference has to fold them again
    with _graph(store), y3.variable_scope('yolov3'):
        model.forward(_data(ia)[0], is_training=True)
    fb3 = infer(ib, 'after a training forward, at (1,96,160)')
    assert not any(torch.equal(a, b) for a, b in zip(fb2, fb3)), 'new moving statistics changed no inference output'


def _oracle_forward(i):
    """fp64 and fp32 training forward of oracle/train_ref.py at SHAPES[i]: feature maps, and the moving statistics after it"""
    if i not in _ORACLE:
        from oracle import train_ref
        x = _data(i)[0].cpu().numpy()
        out = {}
        for dt in (torch.float64, torch.float32):
            g = train_ref.TrainGraph(_params(), CLASS_NUM, dt)
            g.keep_trace = False
            with torch.no_grad():
                fms = [f.double().numpy() for f in g.forward(x)]
            moving = {}
            for name, (mean, _, var_u) in g.batch_stats.items():
                mm, mv = name + '/BatchNorm/moving_mean', name + '/BatchNorm/moving_variance'
                moving[mm] = (g.p[mm] * BN_DECAY + mean * (1 - BN_DECAY)).double().numpy()
                moving[mv] = (g.p[mv] * BN_DECAY + var_u * (1 - BN_DECAY)).double().numpy()
            out[dt] = (fms, moving)
        _ORACLE[i] = out
    return _ORACLE[i]


@pytest.mark.parametrize('dtype', ['f32', 'f32_wino'])
@pytest.mark.parametrize('step', range(len(SHAPES)), ids=['%d-%dx%dx%d' % ((i,) + s) for i, s in enumerate(SHAPES)])
def test_training_forward_at_these_shapes_matches_fp64(step, dtype, isolated_graph):
    """Bit equality with a fresh step leaves "is the fresh step right at these shapes": forward(x, is_training=True) on a
    poisoned workspace against oracle/train_ref.py in fp64.  Feature maps by the rule of test_forward_matches_oracle_416 -
    the GPU's max error at most max(20 x the oracle's own fp32-against-fp64 error, 5e-5) - and the updated moving
    statistics at rtol 1e-5 / atol 1e-6 (test_bn_train_forward_backward).  fp32 modes only: the bf16 gates of
    test_train_bf16_gpu.py are figures measured at 256 px, bs=4 against an oracle that needs that step's LeakyReLU
    branches, and do not transfer to these shapes.  Gradients are left to the seeded oracle tests."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    x = _data(step)[0]
    ref64, ref32 = _oracle_forward(step)[torch.float64], _oracle_forward(step)[torch.float32]
    with _graph({}):
        model = _fresh_model(_params(), CLASS_NUM, batch_norm_decay=BN_DECAY, weight_decay=WEIGHT_DECAY)
        model.compute_dtype = dtype
        with y3.variable_scope('yolov3'):
            st, _, _ = training._prepare(model, x)
            ws = st['ws']
            ws.fill_(0xFF)
            fms = [f.double().cpu().numpy() for f in model.forward(x, is_training=True)]
            assert model._train['ws'] is ws
            got = {v.op_name: v.numpy() for v in y3.global_variables(scope='yolov3') if '/moving_' in v.op_name}
    for k, (g, r64, r32) in enumerate(zip(fms, ref64[0], ref32[0])):
        assert g.shape == r64.shape
        e, e32 = float(np.abs(g - r64).max()), float(np.abs(r32 - r64).max())
        print('%s %s feature_map_%d: GPU-vs-fp64 %.3e ; oracle-fp32-vs-fp64 %.3e' % (dtype, SHAPES[step], k + 1, e, e32))
        assert np.isfinite(g).all()
        assert e <= max(20 * e32, 5e-5), 'GPU drift is far above the fp32 CPU drift'
    assert set(got) == set(ref64[1]) and len(got) == 144
    worst = max(float(np.abs(got[k] - ref64[1][k]).max()) for k in got)
    print('%s %s moving statistics: worst abs error %.3e' % (dtype, SHAPES[step], worst))
    for k in sorted(got):
        np.testing.assert_allclose(got[k], ref64[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
