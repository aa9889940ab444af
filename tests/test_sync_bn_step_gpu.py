"""The batch-norm exchange hook inside the train step (y3_net_train_set_bn_sync, training.Trainer(sync_bn=...)), one process.

No process group here: a distributed.BnSync with its `force` switch set and its `exchange` replaced stands for the collective.
  identity   the buffer left alone: sums | finish must give the bits of the step without a hook - loss, every gradient, every
             moving statistic, in every train mode and with the weight gradients on either stream;
  doubling   `buf.mul_(2)` on the stream: a world of two ranks that hold the SAME batch (exact in fp64).  Means, variances
             and the backward coefficients are quotients of doubled sums by a doubled count, so loss and gradients keep their
             bits - unless d gamma / d beta were taken from the exchanged sums, which would double them - and moving_mean is
             unchanged, while moving_variance carries the unbiased factor of 2 * rows instead of rows.
Also: the order of the hook calls, none below the first trainable layer in backward, and a failing hook."""
import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS, blob_images

pytestmark = pytest.mark.gpu

N, SIZE, DECAY = 2, 96, 0.9


def _conv_name(i):
    sub, j = ('darknet53_body', i) if i < 52 else ('yolov3_head', i - 52)
    return 'yolov3/%s/%s' % (sub, 'Conv' if j == 0 else 'Conv_%d' % j)


def _inputs():
    from oracle import yolo_ref, train_ref
    return (yolo_ref.synthetic_params(80, seed=2), blob_images(4, N, SIZE),
            train_ref.synthetic_targets(6, N, [SIZE, SIZE], 80, COCO_ANCHORS, max_boxes=3))


def _fresh_model(params, dtype):
    import yolov3_tensorflow_amd as y3
    y3.reset_default_graph()
    model = y3.yolov3(80, COCO_ANCHORS, batch_norm_decay=DECAY)
    model.compute_dtype = dtype
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    for v in y3.global_variables(scope='yolov3'):
        v.assign(params[v.op_name])
    return model


def _sync(exchange):
    from yolov3_tensorflow_amd import distributed
    sync = distributed.BnSync()
    sync.force = True
    sync.exchange = lambda doubles: exchange(sync, doubles)
    return sync


def _one_step(inputs, dtype, wgrad_stream, sync, update_prefix=None):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    params, x, yts = inputs
    model = _fresh_model(params, dtype)
    upd = None
    if update_prefix is not None:
        upd = [v for v in y3.global_variables(scope='yolov3') if v.op_name.startswith(update_prefix)]
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), update_vars=upd, wgrad_stream=wgrad_stream, sync_bn=sync)
    with y3.variable_scope('yolov3'):
        loss = [float(v) for v in trainer.step(x, yts)]
    torch.cuda.synchronize()
    moving = {v.op_name: v.numpy().copy() for v in y3.global_variables(scope='yolov3') if '/moving_' in v.op_name}
    return dict(loss=loss, flat=trainer.flat.clone(), moving=moving, model=model, trainer=trainer)


@pytest.mark.parametrize('wgrad_stream', [False, True])
@pytest.mark.parametrize('dtype', ['f32_wino', 'bf16', 'f32_bf16x6'])      # (f32_bf16x6: the split-plane routes, nblk == 0)
def test_identity_and_doubling_hooks_against_the_step_without_a_hook(dtype, wgrad_stream, isolated_graph):
    inputs = _inputs()
    params = inputs[0]
    plain = _one_step(inputs, dtype, wgrad_stream, False)
    assert plain['model']._train.get('bn_sync_cb') is None
    layers = plain['model']._train['topo'].layers
    tensors = plain['model']._train['topo'].tensors
    bn = [i for i, l in enumerate(layers) if l['bn']]
    assert len(bn) == 72

    ident = _one_step(inputs, dtype, wgrad_stream, _sync(lambda s, d: None))
    assert ident['trainer'].bn_sync.calls == [(i, 0) for i in bn] + [(i, 1) for i in reversed(bn)]
    assert ident['loss'] == plain['loss']
    assert torch.equal(ident['flat'], plain['flat'])
    assert set(ident['moving']) == set(plain['moving']) and len(plain['moving']) == 144
    for k, v in plain['moving'].items():
        np.testing.assert_array_equal(ident['moving'][k], v, err_msg=k)

    twice = _one_step(inputs, dtype, wgrad_stream, _sync(lambda s, d: s.buf[:d].mul_(2)))
    assert twice['loss'] == plain['loss']
    assert torch.equal(twice['flat'], plain['flat']), 'a gradient changed under a doubled exchange buffer (d gamma / d beta?)'
    for i in bn:
        name = _conv_name(i) + '/BatchNorm/'
        np.testing.assert_array_equal(twice['moving'][name + 'moving_mean'], plain['moving'][name + 'moving_mean'], err_msg=name)
        # plain: mv' = d mv + (1 - d) var r / (r - 1); with the doubled buffer the factor is 2r / (2r - 1).  Recovering
        # var r / (r - 1) from the fp32 mv' costs about ulp(mv') / (1 - d), which the (1 - d) in front takes back.
        rows = float(N * (SIZE // tensors[layers[i]['dst']]['sdiv']) ** 2)
        mv0 = params[name + 'moving_variance'].astype(np.float64)
        unb = (plain['moving'][name + 'moving_variance'].astype(np.float64) - DECAY * mv0) / (1 - DECAY)
        want = DECAY * mv0 + (1 - DECAY) * unb * (2 * rows / (2 * rows - 1)) / (rows / (rows - 1))
        np.testing.assert_allclose(twice['moving'][name + 'moving_variance'], want, rtol=1e-5, err_msg=name)
    # (the check resolves the factor: at the 3x3 grid, 18 rows, 18/17 against 36/35 is 3 % of the batch variance)
    last = _conv_name(bn[-1]) + '/BatchNorm/moving_variance'
    assert np.abs(twice['moving'][last] - plain['moving'][last]).max() > 1e-4 * np.abs(plain['moving'][last]).max()


def test_backward_calls_the_hook_for_no_layer_below_the_first_trainable_one(isolated_graph):
    inputs = _inputs()
    run = _one_step(inputs, 'f32', True, _sync(lambda s, d: None), update_prefix='yolov3/yolov3_head')
    layers = run['model']._train['topo'].layers
    bn = [i for i, l in enumerate(layers) if l['bn']]
    calls = run['trainer'].bn_sync.calls
    assert calls[:72] == [(i, 0) for i in bn]
    assert calls[72:] == [(i, 1) for i in reversed(bn) if i >= 52] and len(calls) > 72


def test_a_failing_hook_ends_the_step_and_the_next_step_runs(isolated_graph):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import _lib, distributed, framework as fw, training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    params, x, yts = _inputs()

    class Failing(distributed.BnSync):
        fail_at = None          # (layer, phase) at which the hook returns nonzero without an exception

        def __call__(self, layer, phase, doubles):
            if (layer, phase) == self.fail_at:
                return 7
            return distributed.BnSync.__call__(self, layer, phase, doubles)

    sync = Failing()
    sync.force = True
    sync.exchange = lambda doubles: None
    model = _fresh_model(params, 'f32')
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), wgrad_stream=True, sync_bn=sync)
    with y3.variable_scope('yolov3'):
        good = [float(v) for v in trainer.step(x, yts)]
        # a nonzero return in backward, weight gradients in flight on the second stream
        sync.fail_at = (60, 1)
        with pytest.raises(_lib.Y3Error, match='exchange hook'):
            trainer.step(x, yts)
        assert sync.calls[-1] == (61, 1)
        # ... in forward
        sync.fail_at = (5, 0)
        with pytest.raises(_lib.Y3Error, match='exchange hook'):
            trainer.step(x, yts)
        assert sync.calls == [(i, 0) for i in range(5)]
        sync.fail_at = None

        # a Python exception inside the hook comes back as itself
        def boom(doubles):
            if len(sync.calls) == 10:
                raise RuntimeError('collective failed')
        sync.exchange = boom
        with pytest.raises(RuntimeError, match='collective failed'):
            trainer.step(x, yts)
        assert len(sync.calls) == 10 and sync.error is None
        sync.exchange = lambda doubles: None
        again = [float(v) for v in trainer.step(x, yts)]
    assert len(sync.calls) == 144
    assert all(np.isfinite(again)) and all(np.isfinite(good))
    fw.check_context()


def test_the_exchange_buffer_is_checked(isolated_graph):
    import ctypes
    from yolov3_tensorflow_amd import _lib, framework as fw
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(fw.context(), 80, ctypes.byref(h)))
    cb = _lib.BnSyncFn(lambda user, layer, phase, doubles: 0)
    buf = torch.zeros(2 * 1024 + 1, dtype=torch.float64, device=fw.default_device())
    assert L.y3_net_train_set_bn_sync(h, cb, None, fw.ptr(buf), ctypes.c_size_t(2 * 1024 * 8)) == _lib.Y3_EINVAL
    assert L.y3_net_train_set_bn_sync(h, cb, None, None, ctypes.c_size_t(1 << 20)) == _lib.Y3_EINVAL
    assert L.y3_net_train_set_bn_sync(h, cb, None, fw.ptr(buf), ctypes.c_size_t((2 * 1024 + 1) * 8)) == _lib.Y3_OK
    assert L.y3_net_train_set_bn_sync(h, _lib.BnSyncFn(), None, None, 0) == _lib.Y3_OK      # off again
    _lib.check(L.y3_net_destroy(h))
