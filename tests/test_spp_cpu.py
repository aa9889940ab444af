"""CPU tests of the YOLOv3-SPP feature: the kernels' per-element rules (csrc/y3_spp_px.h) run on the host in the kernels' order
(tests/spp_emul.cpp) against torch and the ordered fp32 sum; the 76-layer graph through a net without a context; the variable
table, the darknet import and the checkpoint rule.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import spp_cases as sc
from conftest import COCO_ANCHORS, ROOT


# ---- the rules on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('spp_emul') / 'libspp_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-Wall',
                           os.path.join(ROOT, 'tests', 'spp_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3spp_emul_fwd.restype = ctypes.c_int
    lib.y3spp_emul_fwd.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.y3spp_emul_bwd.restype = ctypes.c_int
    lib.y3spp_emul_bwd.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 5 + [
        ctypes.c_void_p]
    return lib


def _emul_fwd(emul, x):
    """x: contiguous NHWC torch tensor, float32 or bfloat16"""
    n, h, w, c = x.shape
    out = torch.empty((n, h, w, 4 * c), dtype=x.dtype)
    assert emul.y3spp_emul_fwd(x.data_ptr(), int(x.dtype == torch.bfloat16), n, h, w, c, out.data_ptr()) == 0
    return out


def _emul_bwd(emul, x, g, dx0=None):
    n, h, w, c = x.shape
    dx = torch.full((n, h, w, c), float('nan')) if dx0 is None else torch.from_numpy(dx0.copy())
    g = torch.from_numpy(g)
    assert emul.y3spp_emul_bwd(x.data_ptr(), c, int(x.dtype == torch.bfloat16), g.data_ptr(), n, h, w, c, int(dx0 is not None),
                               dx.data_ptr()) == 0
    return dx.numpy()


@pytest.mark.parametrize('kind', ['continuous', 'ties'])
@pytest.mark.parametrize('shape', sc.CPU_SHAPES, ids=str)
def test_forward_rules_equal_torch_bit_for_bit(emul, shape, kind):
    x = torch.from_numpy(sc.inputs(kind, shape, seed=3))
    for t in (x, x.to(torch.bfloat16)):
        got, want = _emul_fwd(emul, t.contiguous()), sc.spp_ref(t)
        assert torch.equal(got.view(torch.int32 if t.dtype == torch.float32 else torch.int16),
                           want.view(torch.int32 if t.dtype == torch.float32 else torch.int16)), t.dtype


def test_pool_compositions_hold_exactly():
    """mp_9 = mp_5 o mp_5 and mp_13 = mp_5 o mp_5 o mp_5 with padding that never wins (what the forward kernel uses)"""
    import torch.nn.functional as F
    for kind in ('continuous', 'ties'):
        x = torch.from_numpy(sc.inputs(kind, (2, 19, 20, 8), seed=5)).permute(0, 3, 1, 2)
        p5 = F.max_pool2d(x, 5, 1, 2)
        p9 = F.max_pool2d(p5, 5, 1, 2)
        assert torch.equal(p9, F.max_pool2d(x, 9, 1, 4))
        assert torch.equal(F.max_pool2d(p9, 5, 1, 2), F.max_pool2d(x, 13, 1, 6))


def test_first_max_rule_is_torchs():
    """torch's CPU max_pool2d sends a window's gradient to its first maximum in row-major order: an all-zero 5x5 map sends the
    corner window's whole gradient to the top-left element; and spp_cases.first_argmax is that rule on a tie-heavy map"""
    import torch.nn.functional as F
    x = torch.zeros(1, 1, 5, 5, requires_grad=True)
    g = torch.zeros(1, 1, 5, 5)
    g[0, 0, 0, 0] = 1.0
    F.max_pool2d(x, 5, 1, 2).backward(g)
    assert float(x.grad[0, 0, 0, 0]) == 1.0 and float(x.grad.abs().sum()) == 1.0
    xt = sc.inputs('ties', (2, 7, 5, 16), seed=7)
    for k in sc.WINDOWS:
        _, idx = F.max_pool2d(torch.from_numpy(xt).permute(0, 3, 1, 2), k, 1, k // 2, return_indices=True)
        ay, ax = sc.first_argmax(xt, k)
        np.testing.assert_array_equal(idx.permute(0, 2, 3, 1).numpy(), ay * 5 + ax)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('kind', ['continuous', 'ties'])
@pytest.mark.parametrize('shape', sc.CPU_SHAPES, ids=str)
def test_backward_rules_equal_the_ordered_sum_and_stay_within_the_fp64_bound(emul, shape, kind, bf16, accumulate):
    xn = sc.inputs(kind, shape, seed=11)
    g = sc.gradients(shape, seed=12)
    dx0 = np.random.RandomState(13).standard_normal(shape).astype(np.float32) if accumulate else None
    x = torch.from_numpy(xn)
    got = _emul_bwd(emul, (x.to(torch.bfloat16) if bf16 else x).contiguous(), g, dx0)
    want = sc.bwd_ordered(xn, g, dx0)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    # against torch's fp64 autograd: at most 276 terms reach one element, each addition rounds once
    ref, sum_abs = sc.bwd_fp64(xn, g)
    if accumulate:
        ref, sum_abs = ref + dx0.astype(np.float64), sum_abs + np.abs(dx0.astype(np.float64))
    bound = sc.MAX_TERMS * 2.0 ** -24 * sum_abs
    assert sc.MAX_TERMS == 276
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), float((np.abs(got - ref) - bound).max())


def test_backward_reads_a_strided_x(emul):
    """x as the last slot of a materialised spp(x): x + 3c, stride 4c"""
    shape = (2, 7, 5, 16)
    n, h, w, c = shape
    xn = sc.inputs('ties', shape, seed=21)
    g = sc.gradients(shape, seed=22)
    pooled = sc.spp_ref(torch.from_numpy(xn)).contiguous()
    dx = torch.empty(shape)
    gt = torch.from_numpy(g)
    assert emul.y3spp_emul_bwd(pooled.data_ptr() + 3 * c * 4, 4 * c, 0, gt.data_ptr(), n, h, w, c, 0, dx.data_ptr()) == 0
    np.testing.assert_array_equal(dx.numpy().view(np.int32), sc.bwd_ordered(xn, g).view(np.int32))


def test_oracle_with_an_imposed_argmax_is_the_oracle_on_its_own_comparison():
    """SppTrainGraph reads the window maxima at imposed positions (a gather); with the first-max positions of its own pool
    input that is its own max_pool2d path: same loss, same gradients (fp64, 96 x 96: a 3 x 3 grid)"""
    from oracle import train_ref
    params = sc.spp_params(80, seed=1)
    rng = np.random.RandomState(0)
    x = rng.rand(2, 96, 96, 3).astype(np.float32)
    yts = train_ref.synthetic_targets(5, 2, [96, 96], 80, COCO_ANCHORS, max_boxes=3)
    names = {'yolov3/yolov3_head/Conv_2/weights', 'yolov3/yolov3_head/Conv_3/weights', 'yolov3/darknet53_body/Conv_51/BatchNorm/gamma'}
    own = sc.train_step(params, x, yts, COCO_ANCHORS, update_names=names)
    pooled_in = own['graph'].pool_input.permute(0, 2, 3, 1).numpy()
    assert pooled_in.shape == (2, 3, 3, 512)
    argmax = {k: sc.first_argmax(pooled_in, k) for k in sc.WINDOWS}
    imposed = sc.train_step(params, x, yts, COCO_ANCHORS, update_names=names, pool_argmax=argmax)
    # (the gathered tensor has another memory layout than max_pool2d's: the convs behind it may sum in another order)
    np.testing.assert_allclose(imposed['loss'], own['loss'], rtol=1e-12)
    assert set(own['grads']) == names
    for k in names:
        scale = np.abs(own['grads'][k]).max()
        assert scale > 0 and np.abs(imposed['grads'][k] - own['grads'][k]).max() <= 1e-10 * scale, k


# ---- the graph, through a net without a context ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _net(lib, arch=None, class_num=80):
    from yolov3_tensorflow_amd import _lib
    h = ctypes.c_void_p()
    if arch is None:
        _lib.check(lib.y3_net_create(None, class_num, ctypes.byref(h)))
    else:
        _lib.check(lib.y3_net_create_arch(None, class_num, arch, ctypes.byref(h)))
    return h


def _tables(lib, h):
    ci = ctypes.c_int
    layers, tensors = [], []
    for i in range(lib.y3_net_num_layers(h)):
        a = [ci() for _ in range(10)]
        assert lib.y3_net_layer_info(h, i, *[ctypes.byref(v) for v in a[:5]]) == 0
        assert lib.y3_net_layer_graph(h, i, *[ctypes.byref(v) for v in a[5:]]) == 0
        layers.append(tuple(v.value for v in a) + (lib.y3_net_layer_pool(h, i),))
    for t in range(lib.y3_net_num_tensors(h)):
        a = [ci() for _ in range(3)]
        assert lib.y3_net_tensor_info(h, t, *[ctypes.byref(v) for v in a]) == 0
        tensors.append(tuple(v.value for v in a))
    return layers, tensors


def test_spp_architecture_has_76_layers_and_one_pool_layer(lib):
    h = _net(lib, 1)
    assert lib.y3_net_arch(h) == 1
    layers, tensors = _tables(lib, h)
    assert len(layers) == 76 and len(tensors) == 77
    assert sum(l[4] for l in layers) == 73            # with BN
    assert [i for i, l in enumerate(layers) if l[10]] == [55]
    # (k, stride, cin, cout, bn) of the changed block: 1x1 512, 3x3 1024, 1x1 512, SPP, 1x1 512 (Cin = 2048), 3x3 1024, 1x1 512, 3x3 1024
    assert [l[:5] for l in layers[52:60]] == [(1, 1, 1024, 512, 1), (3, 1, 512, 1024, 1), (1, 1, 1024, 512, 1), (1, 1, 2048, 512, 1),
                                              (3, 1, 512, 1024, 1), (1, 1, 1024, 512, 1), (3, 1, 512, 1024, 1), (1, 1, 1024, 255, 0)]
    # tensor id == layer index + 1; the pool layer reads the conv before it and has neither a concat nor a shortcut input
    assert all(l[8] == i + 1 for i, l in enumerate(layers))
    assert layers[55][5:8] == (55, -1, -1) and tensors[55][0] == 512
    # the route of the 13-grid is the 1x1 two layers later: the 26-grid's lateral conv reads it
    assert layers[60][5] == 58 and layers[60][:5] == (1, 1, 512, 256, 1)
    # everything else is the default graph, shifted by one behind the block
    d_layers, _ = _tables(lib, _net(lib))
    assert layers[:52] == d_layers[:52]
    shift = lambda t: t + 1 if t >= 56 else t
    for a, b in zip(layers[59:], d_layers[58:]):
        assert a[:5] == b[:5] and a[9:] == b[9:]
        assert a[5:9] == tuple(shift(t) if t >= 0 else t for t in b[5:9])
    assert lib.y3_net_workspace_bytes(h, 2, 64, 64) > 0
    lib.y3_net_destroy(h)


def test_architecture_0_is_y3_net_create(lib):
    a, b = _net(lib), _net(lib, 0)
    assert lib.y3_net_arch(a) == 0 and lib.y3_net_arch(b) == 0
    assert _tables(lib, a) == _tables(lib, b)
    assert len(_tables(lib, a)[0]) == 75 and not any(l[10] for l in _tables(lib, a)[0])
    for dtype in (0, 1, 4):
        assert lib.y3_net_set_dtype(a, dtype) == 0 and lib.y3_net_set_dtype(b, dtype) == 0
        for n, h, w in ((32, 416, 416), (16, 608, 608)):
            assert lib.y3_net_workspace_bytes(a, n, h, w) == lib.y3_net_workspace_bytes(b, n, h, w) > 0
    lib.y3_net_destroy(a)
    lib.y3_net_destroy(b)


def test_unknown_architecture_is_einval_and_the_abi_version_is_5(lib):
    from yolov3_tensorflow_amd import _lib
    h = ctypes.c_void_p()
    for arch in (-1, 2, 7):
        assert lib.y3_net_create_arch(None, 80, arch, ctypes.byref(h)) == _lib.Y3_EINVAL
        assert b'architecture' in lib.y3_last_error()
    assert lib.y3_abi_version() == 5
    assert lib.y3_net_layer_pool(None, 0) == 0


def test_spp_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """(no context exists here: a null context is itself a bad argument, and the checks come before any launch)"""
    from yolov3_tensorflow_amd import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.y3_spp_fwd(None, p, 0, 1, 1, 1, 8, p) == _lib.Y3_EINVAL
    assert lib.y3_spp_bwd(None, p, 8, 0, p, 1, 1, 1, 8, 0, p) == _lib.Y3_EINVAL


# ---- variables and weights ---------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_variables(isolated_graph):
    """Variables on the CPU (the store needs a device; none of the tests below launches anything)"""
    from yolov3_tensorflow_amd import framework as fw
    saved = fw._default_device[0]
    fw.set_default_device('cpu')
    try:
        yield
    finally:
        fw._default_device[0] = saved


def _make_variables(spp, class_num=80):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    model = y3.yolov3(class_num, COCO_ANCHORS)
    model.spp = spp
    topo = training._Topology(class_num, training._arch(model))
    table = [(l['k'], l['stride'], l['cin'], l['cout'], l['bn']) for l in topo.layers]
    model._ensure_variables('yolov3', table)
    return y3.global_variables(scope='yolov3')


def test_spp_model_has_371_variables_under_the_shifted_names(lib, cpu_variables):
    variables = _make_variables(True)
    want = sc.spp_params(80, seed=1)
    assert len(variables) == 371 == len(want)
    assert [v.op_name for v in variables] == list(want)
    assert [tuple(v.shape) for v in variables] == [tuple(a.shape) for a in want.values()]
    names = [v.op_name for v in variables]
    assert 'yolov3/yolov3_head/Conv_23/weights' in names and 'yolov3/yolov3_head/Conv_24/weights' not in names
    assert sum(1 for v in variables if v.trainable) == 225
    assert not any('darknet53_body/Conv_52' in nm for nm in names)       # the body stays 52 convs


def test_default_model_keeps_its_366_variables(lib, cpu_variables):
    from oracle import yolo_ref
    variables = _make_variables(False)
    assert [v.op_name for v in variables] == [n for n, _ in yolo_ref.variable_specs(80)] and len(variables) == 366


def test_darknet_file_in_graph_order_round_trips_through_load_weights(lib, cpu_variables, tmp_path):
    from oracle import yolo_ref
    from yolov3_tensorflow_amd.utils.misc_utils import load_weights, run_ops
    params = sc.spp_params(80, seed=2)
    path = str(tmp_path / 'yolov3-spp.weights')
    yolo_ref.write_darknet(params, path)        # numpy, in graph order
    variables = _make_variables(True)
    run_ops(load_weights(variables, path))
    for v in variables:
        np.testing.assert_array_equal(v.numpy(), params[v.op_name], err_msg=v.op_name)
    # the default architecture's file does not fit the SPP variable list
    small = str(tmp_path / 'yolov3.weights')
    yolo_ref.write_darknet(yolo_ref.synthetic_params(80, seed=2), small)
    with pytest.raises(ValueError):
        run_ops(load_weights(variables, small))


def test_default_checkpoint_into_an_spp_model_fails_on_the_first_changed_variable(lib, cpu_variables, tmp_path):
    from oracle import yolo_ref
    from yolov3_tensorflow_amd.utils.misc_utils import Saver
    default = yolo_ref.synthetic_params(80, seed=3)
    path = str(tmp_path / 'default.npz')
    with open(path, 'wb') as f:
        np.savez(f, **default)                  # a whole default-architecture checkpoint, keyed by name as the Saver writes it
    variables = _make_variables(True)
    with pytest.raises(ValueError) as err:
        Saver(variables).restore(path)
    assert 'yolov3/yolov3_head/Conv_3/weights' in str(err.value)
    # restoring only the body works: its names and shapes are the default architecture's
    body = [v for v in variables if v.op_name.startswith('yolov3/darknet53_body')]
    Saver(body).restore(path)
    for v in body:
        np.testing.assert_array_equal(v.numpy(), default[v.op_name], err_msg=v.op_name)
