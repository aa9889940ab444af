"""The conv route table of the net: which kernel form each layer takes, as the host queries of the C ABI report it, for every
net dtype at several input shapes.  Host-only calls on a net created without a context (no GPU):

    python tests/golden/make_route_golden.py [--device]       ->  tests/golden/conv_routes.json

Some entries depend on the device the library sees (the fused stem / residual block need the device to offer their kernels'
LDS), so the file holds two tables: 'host' (made without a device) and 'device' (made on an MI355X, --device).

Per (dtype, n, h, w) it records, per layer, y3_net_layer_fused, y3_net_layer_is_streamk and
y3_conv_bf16_tile of the layer's descriptor; y3_net_workspace_bytes; and, for the train dtypes (0, 2, 3, 4),
y3_net_train_workspace_bytes with every variable trainable, the weight-gradient stream off and on.  For every dtype at the
SEL_SHAPES, 'train_workspace_sel' holds the same pair for the all-trainable table and for every partial update_vars of
tests/test_train_gpu.py (SELECTIONS): the allocation sequence of backward changes with the selection.
tests/test_conv_route_cpu.py holds the library against the file.  Y3_LIB_PATH selects the library it is made from.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(1, os.path.dirname(HERE))      # (tests/: SELECTIONS of test_train_gpu.py)

OUT = os.path.join(HERE, 'conv_routes.json')
SHAPES = ((32, 416, 416), (16, 608, 608), (64, 416, 416), (4, 256, 256), (3, 320, 320), (2, 416, 608), (1, 96, 96),
          (8, 416, 416))
TRAIN_DTYPES = (0, 2, 3, 4)
SEL_SHAPES = ((1, 96, 96), (4, 256, 256), (3, 320, 320), (2, 416, 608), (8, 416, 416))
CLASS_NUM = 80


class _Var(object):
    """What training.gradient_layout / _var_table read of a variable: name, shape, flag and a storage pointer (a meta
    tensor: the dry run dereferences no pointer)."""

    def __init__(self, op_name, shape, trainable=True):
        import torch
        self.op_name, self.shape, self.trainable = op_name, tuple(shape), trainable
        self.tensor = torch.empty(shape, device='meta')


def layer_vars():
    from yolov3_tensorflow_amd import training
    out = []
    for i, l in enumerate(training._Topology(CLASS_NUM).layers):
        w = _Var('conv%d/weights' % i, (l['k'], l['k'], l['cin'], l['cout']))
        if l['bn']:
            out.append((w, tuple(_Var('conv%d/%s' % (i, s), (l['cout'],), trainable=s in ('gamma', 'beta'))
                                 for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')), None))
        else:
            out.append((w, None, _Var('conv%d/biases' % i, (l['cout'],))))
    return out


def selection_tables():
    """{name: y3_train_var table} of every partial update_vars of tests/test_train_gpu.py, built as
    tests/test_train_workspace_cpu.py builds them (the variables under the names those prefixes select)"""
    import torch
    from yolov3_tensorflow_amd import training
    from test_train_gpu import SELECTIONS, _conv_name
    lvs = []
    for i, l in enumerate(training._Topology(CLASS_NUM).layers):
        base = _conv_name(i)
        w = _Var(base + '/weights', (l['k'], l['k'], l['cin'], l['cout']))
        if l['bn']:
            lvs.append((w, tuple(_Var(base + '/BatchNorm/' + s, (l['cout'],), trainable=s in ('gamma', 'beta'))
                                 for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')), None))
        else:
            lvs.append((w, None, _Var(base + '/biases', (l['cout'],))))
    out = {}
    for name, prefixes in sorted(SELECTIONS.items()):
        picked = [v for lv in lvs for v in (lv[0],) + tuple(lv[1] or ()) + ((lv[2],) if lv[2] else ())
                  if any(v.op_name.startswith(p) for p in prefixes)]
        trainer = training.Trainer(None, None, update_vars=picked)
        trainer._alloc_grads(lvs, torch.device('cpu'))
        out[name] = training._var_table(lvs, trainer.offsets, trainer.layer_ends)
    return out


def descs(L, h, n, H, W):
    """the y3_conv_desc of every layer at input n x H x W (y3_net_forward's: c_up and act included)"""
    from yolov3_tensorflow_amd import _lib
    ci = ctypes.c_int
    out = []
    for i in range(L.y3_net_num_layers(h)):
        k, s, cin, cout, bn = ci(), ci(), ci(), ci(), ci()
        _lib.check(L.y3_net_layer_info(h, i, *[ctypes.byref(v) for v in (k, s, cin, cout, bn)]))
        src, up, resid, dst, act = ci(), ci(), ci(), ci(), ci()
        _lib.check(L.y3_net_layer_graph(h, i, *[ctypes.byref(v) for v in (src, up, resid, dst, act)]))
        sdiv, c_up = ci(), ci(0)
        _lib.check(L.y3_net_tensor_info(h, src.value, None, ctypes.byref(sdiv), None))
        if up.value >= 0:
            _lib.check(L.y3_net_tensor_info(h, up.value, ctypes.byref(c_up), None, None))
        out.append(_lib.ConvDesc(n, H // sdiv.value, W // sdiv.value, cin.value, c_up.value, cout.value, k.value, s.value,
                                 act.value))
    return out


def table():
    """{key: entry} for every case; key = 'dtype<d>/<n>x<h>x<w>' ('dtype4+alt/...' for dtype 4)"""
    from yolov3_tensorflow_amd import _lib, training
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, CLASS_NUM, ctypes.byref(h)))
    all_table, _ = training._var_table(layer_vars())
    sel = dict(selection_tables(), all=(all_table, None))
    nl = L.y3_net_num_layers(h)
    dummy = ctypes.c_void_p(0x1000)      # a weight-gradient stream: the dry run only asks whether there is one
    out = {}
    try:
        for dtype in (0, 1, 2, 3, 4):
            _lib.check(L.y3_net_set_dtype(h, dtype))
            for n, H, W in SHAPES:
                ds = descs(L, h, n, H, W)
                e = {
                    'fused': [L.y3_net_layer_fused(h, i, n, H, W) for i in range(nl)],
                    'streamk': [L.y3_net_layer_is_streamk(h, i, n, H, W) for i in range(nl)],
                    'bf16_tile': ''.join(chr(L.y3_conv_bf16_tile(ctypes.byref(d))) for d in ds),
                    'workspace': L.y3_net_workspace_bytes(h, n, H, W),
                }
                if dtype in TRAIN_DTYPES:
                    ws = []
                    for side in (None, dummy):
                        _lib.check(L.y3_net_train_set_wgrad_stream(h, side))
                        ws.append(L.y3_net_train_workspace_bytes(h, all_table, n, H, W))
                    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))
                    e['train_workspace'] = ws
                if (n, H, W) in SEL_SHAPES:
                    e['train_workspace_sel'] = {}
                    for name in sorted(sel):
                        ws = []
                        for side in (None, dummy):
                            _lib.check(L.y3_net_train_set_wgrad_stream(h, side))
                            ws.append(L.y3_net_train_workspace_bytes(h, sel[name][0], n, H, W))
                        e['train_workspace_sel'][name] = ws
                    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))
                # (dtype 4 keeps the '+alt' of the tables made while its F(4x4,3x3) packings were optional: the net now has them)
                out['dtype%d%s/%dx%dx%d' % (dtype, '+alt' if dtype == 4 else '', n, H, W)] = e
    finally:
        L.y3_net_destroy(h)
    return out


def write(data, out=OUT):
    with open(out, 'w') as f:
        f.write('{\n' + ',\n'.join(
            '%s: {\n' % json.dumps(s) + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(t[k], sort_keys=True)) for k in sorted(t)) + '\n}'
            for s, t in sorted(data.items())) + '\n}\n')


def main():
    """writes the 'host' table, or with --device (run on an MI355X) the 'device' one; -o FILE: write there"""
    section = 'device' if '--device' in sys.argv else 'host'
    out = sys.argv[sys.argv.index('-o') + 1] if '-o' in sys.argv else OUT
    data = {}
    if os.path.exists(out):
        with open(out) as f:
            data = json.load(f)
    data[section] = table()
    write(data, out)
    print('wrote the %s table to %s (%d cases)' % (section, out, len(data[section])))


if __name__ == '__main__':
    main()
