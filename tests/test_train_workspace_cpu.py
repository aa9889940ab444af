"""The train step's workspace for a partial update_vars (ref: train.py --update_part, variables_to_restore on name prefixes).

training._prepare sizes ONE workspace per (shape, device, dtype) with the all-trainable variable table and calls that an
upper bound for any subset.  The allocation sequence of backward does change with the subset (a layer whose gamma / beta
do not train takes a scratch for dgamma / dbeta; only the layers on the second stream defer their releases; the best-fit
free list sees another history), and y3_net_train_forward refuses a workspace below the dry-run peak of the REAL table.
y3_net_train_workspace_bytes is that dry run - host arithmetic, nothing launched, no device needed - so the bound is
checked here for every selection of tests/test_train_gpu.py, both stream settings and the three fp32 compute modes."""
import ctypes

import pytest
import torch

from test_train_gpu import SELECTIONS, _conv_name


class _Var(object):
    """What training.gradient_layout / _var_table / Trainer read of a variable: name, shape, flag and a storage pointer
    (a meta tensor: shape without memory; the dry run dereferences no pointer)."""

    def __init__(self, op_name, shape, trainable=True):
        self.op_name, self.shape, self.trainable = op_name, tuple(shape), trainable
        self.tensor = torch.empty(shape, device='meta')


@pytest.fixture(scope='module')
def net_and_vars():
    from yolov3_tensorflow_amd import build, training, _lib
    build.build(verbose=False)
    L = _lib.lib()
    topo = training._Topology(80)
    layer_vars = []
    for i, l in enumerate(topo.layers):
        base = _conv_name(i)
        w = _Var(base + '/weights', (l['k'], l['k'], l['cin'], l['cout']))
        if l['bn']:
            bn = tuple(_Var(base + '/BatchNorm/' + s, (l['cout'],), trainable=s in ('gamma', 'beta'))
                       for s in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
            layer_vars.append((w, bn, None))
        else:
            layer_vars.append((w, None, _Var(base + '/biases', (l['cout'],))))
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, 80, ctypes.byref(h)))      # no context: sizing only
    yield L, h, layer_vars
    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))
    L.y3_net_destroy(h)


@pytest.mark.parametrize('dtype', ['f32', 'f32_wino', 'f32_bf16x6'])
@pytest.mark.parametrize('n,size', [(4, 256), (8, 416)])
def test_the_all_trainable_workspace_bounds_every_selection(net_and_vars, dtype, n, size):
    from yolov3_tensorflow_amd import training, _lib
    L, h, layer_vars = net_and_vars
    _lib.check(L.y3_net_set_dtype(h, training._TRAIN_DTYPES[dtype]))
    all_table, _ = training._var_table(layer_vars)
    # off, and on: any non-null stream handle (the dry run only asks whether there is one)
    for side in (None, ctypes.c_void_p(0x1000)):
        _lib.check(L.y3_net_train_set_wgrad_stream(h, side))
        bound = L.y3_net_train_workspace_bytes(h, all_table, n, size, size)
        assert bound > 0, L.y3_last_error()
        for name, prefixes in sorted(SELECTIONS.items()):
            picked = [v for lv in layer_vars for v in (lv[0],) + tuple(lv[1] or ()) + ((lv[2],) if lv[2] else ())
                      if any(v.op_name.startswith(p) for p in prefixes)]
            trainer = training.Trainer(None, None, update_vars=picked)
            trainer._alloc_grads(layer_vars, torch.device('cpu'))
            assert trainer.layer_ends, name
            table, _ = training._var_table(layer_vars, trainer.offsets, trainer.layer_ends)
            need = L.y3_net_train_workspace_bytes(h, table, n, size, size)
            assert 0 < need <= bound, '%s, %s, stream %s, %d x %d: subset needs %d bytes, the workspace has %d' % (
                name, dtype, 'on' if side else 'off', n, size, need, bound)
