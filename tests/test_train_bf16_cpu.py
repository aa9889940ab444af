"""The bf16 train step's host side, no device needed: the compute mode, the workspace dry run for net dtype 1 (bf16 saved
tensors: well below the fp32 modes' workspace), the all-trainable bound over partial update_vars, and the saved-z types."""
import ctypes

import pytest

from test_train_gpu import SELECTIONS
from test_train_workspace_cpu import net_and_vars  # noqa: F401  (the fixture: a net without a context, meta variables)

SHAPES = [(1, 32), (2, 64), (4, 256), (8, 416), (16, 608), (64, 416)]


def test_bf16_is_a_train_mode():
    from yolov3_tensorflow_amd import training
    assert training._TRAIN_DTYPES['bf16'] == 1


def test_bf16_workspace_at_every_shape_and_against_fp32(net_and_vars):
    from yolov3_tensorflow_amd import training, _lib
    L, h, layer_vars = net_and_vars
    table, _ = training._var_table(layer_vars)
    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))
    for n, size in SHAPES:
        _lib.check(L.y3_net_set_dtype(h, 1))
        b = L.y3_net_train_workspace_bytes(h, table, n, size, size)
        assert b > 0, (n, size, L.y3_last_error())
        if (n, size) == (64, 416):
            _lib.check(L.y3_net_set_dtype(h, 0))
            f = L.y3_net_train_workspace_bytes(h, table, n, size, size)
            print('train workspace at 64 x 416: bf16 %.2f GB, f32 %.2f GB, ratio %.3f' % (b / 1e9, f / 1e9, b / f))
            assert b <= 0.7 * f


@pytest.mark.parametrize('n,size', [(4, 256), (8, 416)])
def test_the_all_trainable_bf16_workspace_bounds_every_selection(net_and_vars, n, size):
    from yolov3_tensorflow_amd import training, _lib
    L, h, layer_vars = net_and_vars
    _lib.check(L.y3_net_set_dtype(h, training._TRAIN_DTYPES['bf16']))
    all_table, _ = training._var_table(layer_vars)
    for side in (None, ctypes.c_void_p(0x1000)):
        _lib.check(L.y3_net_train_set_wgrad_stream(h, side))
        bound = L.y3_net_train_workspace_bytes(h, all_table, n, size, size)
        assert bound > 0, L.y3_last_error()
        for name, prefixes in sorted(SELECTIONS.items()):
            picked = [v for lv in layer_vars for v in (lv[0],) + tuple(lv[1] or ()) + ((lv[2],) if lv[2] else ())
                      if any(v.op_name.startswith(p) for p in prefixes)]
            trainer = training.Trainer(None, None, update_vars=picked)
            trainer._alloc_grads(layer_vars, __import__('torch').device('cpu'))
            table, _ = training._var_table(layer_vars, trainer.offsets, trainer.layer_ends)
            need = L.y3_net_train_workspace_bytes(h, table, n, size, size)
            assert 0 < need <= bound, (name, 'on' if side else 'off', n, size, need, bound)
    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))


def test_saved_z_types(net_and_vars):
    from yolov3_tensorflow_amd import training, _lib
    L, h, _ = net_and_vars
    topo = training._Topology(80)
    _lib.check(L.y3_net_set_dtype(h, 1))
    for i, l in enumerate(topo.layers):
        assert L.y3_net_train_saved_type(h, i) == (1 if l['bn'] and i > 0 else 0), i
    _lib.check(L.y3_net_set_dtype(h, 0))
    assert all(L.y3_net_train_saved_type(h, i) == 0 for i in range(len(topo.layers)))
