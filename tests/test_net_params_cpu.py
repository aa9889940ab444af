"""The inference net's parameter buffer (y3_net_params_bytes / y3_net_set_params): its size per dtype, computed here on its own
from the layer table and the exported eligibility predicates, and the argument checks of the call.  Host-only (no GPU)."""
import ctypes

import pytest

CLASS_NUM = 80


@pytest.fixture(scope='module')
def lib():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture
def net(lib):
    h = ctypes.c_void_p()
    assert lib.y3_net_create(None, CLASS_NUM, ctypes.byref(h)) == 0
    yield h
    lib.y3_net_destroy(h)


def layers(lib, h):
    """per layer: k, stride, cin, cout and the spatial divisor of its input"""
    ci = ctypes.c_int
    out = []
    for i in range(lib.y3_net_num_layers(h)):
        k, s, cin, cout, bn, src, sdiv = ci(), ci(), ci(), ci(), ci(), ci(), ci()
        assert lib.y3_net_layer_info(h, i, *[ctypes.byref(v) for v in (k, s, cin, cout, bn)]) == 0
        assert lib.y3_net_layer_graph(h, i, ctypes.byref(src), None, None, None, None) == 0
        assert lib.y3_net_tensor_info(h, src.value, None, ctypes.byref(sdiv), None) == 0
        out.append((k.value, s.value, cin.value, cout.value, sdiv.value))
    return out


def expected_bytes(lib, h, dtype):
    """per layer: scale and shift, then the kernel in every packing the dtype's inference kernels may read; each region rounded
    up to 256 bytes.  dtype 4: F(2x2,3x3) where the Winograd kernel takes the layer, the direct packing where it refuses it at
    the smallest legal input (32 x 32: the /32 map is 1 x 1), F(4x4,3x3) where y3_conv_wino44_candidate holds."""
    from yolov3_tensorflow_amd import _lib
    rnd = lambda b: (b + 255) // 256 * 256
    total, both = 0, 0
    for k, s, cin, cout, sdiv in layers(lib, h):
        taps = k * k * cin * cout
        total += 2 * rnd(4 * cout)
        if cin == 3:                              # the stem: its HWIO kernel, copied
            total += rnd(4 * taps)
        elif dtype == 0:
            total += rnd(4 * taps)
        elif dtype == 1:
            total += rnd(2 * taps)
        elif dtype in (2, 3):
            total += rnd(2 * (3 if dtype == 2 else 2) * taps)
        else:
            small = _lib.ConvDesc(1, 32 // sdiv, 32 // sdiv, cin, 0, cout, k, s, 1)
            large = _lib.ConvDesc(1, 64 // sdiv, 64 // sdiv, cin, 0, cout, k, s, 1)
            wino = lib.y3_conv_wino_eligible(ctypes.byref(large)) == 1
            direct = lib.y3_conv_wino_eligible(ctypes.byref(small)) != 1
            both += wino and direct
            total += (rnd(16 * cin * cout * 4) if wino else 0) + (rnd(4 * taps) if direct else 0)
            if lib.y3_conv_wino44_candidate(ctypes.byref(large)) == 1:
                total += rnd(36 * cin * cout * 4)
    if dtype == 4:
        assert both == 7           # the 3x3 stride-1 convs of the /32 map
    return total


@pytest.mark.parametrize('dtype', [0, 1, 2, 3, 4])
def test_params_bytes_per_dtype(lib, net, dtype):
    assert lib.y3_net_set_dtype(net, dtype) == 0
    assert lib.y3_net_params_bytes(net) == expected_bytes(lib, net, dtype)


def test_set_params_checks_its_arguments(lib, net):
    from yolov3_tensorflow_amd import _lib
    assert lib.y3_net_params_bytes(None) == 0
    assert lib.y3_net_set_dtype(net, 4) == 0
    nbytes = lib.y3_net_params_bytes(net)
    fake = ctypes.c_void_p(1 << 20)               # binding only: the host touches no parameter memory
    assert lib.y3_net_set_params(net, None, fake, ctypes.c_size_t(nbytes - 1)) == _lib.Y3_EINVAL
    assert lib.y3_net_set_params(net, None, ctypes.c_void_p((1 << 20) + 16), ctypes.c_size_t(nbytes)) == _lib.Y3_EINVAL
    assert lib.y3_net_set_params(net, None, fake, ctypes.c_size_t(nbytes)) == 0
    # packing needs a context; the net was created without one
    vars_ = (_lib.TrainVar * lib.y3_net_num_layers(net))()
    assert lib.y3_net_set_params(net, vars_, fake, ctypes.c_size_t(nbytes)) == _lib.Y3_ESTATE
