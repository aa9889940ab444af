#!/usr/bin/env python
"""y3_net_train_workspace_bytes for every net dtype, a spread of shapes, both stream settings and every variable selection of
tests/test_train_workspace_cpu.py, one line each: run it on two builds (Y3_LIB_PATH picks the library) and diff the output to
show that a change left the allocation sequence of the train step alone.  Host only, no GPU."""
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_train_gpu import SELECTIONS, _conv_name  # noqa: E402
from test_train_workspace_cpu import _Var  # noqa: E402
from yolov3_tensorflow_amd import _lib, training  # noqa: E402


def main():
    L = _lib.lib()
    topo = training._Topology(80)
    layer_vars = []
    for i, l in enumerate(topo.layers):
        base = _conv_name(i)
        w = _Var(base + '/weights', (l['k'], l['k'], l['cin'], l['cout']))
        if l['bn']:
            layer_vars.append((w, tuple(_Var(base + '/BatchNorm/' + s, (l['cout'],), trainable=s in ('gamma', 'beta'))
                                        for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')), None))
        else:
            layer_vars.append((w, None, _Var(base + '/biases', (l['cout'],))))
    tables = {'all': training._var_table(layer_vars)[0]}
    for name, prefixes in sorted(SELECTIONS.items()):
        picked = [v for lv in layer_vars for v in (lv[0],) + tuple(lv[1] or ()) + ((lv[2],) if lv[2] else ())
                  if any(v.op_name.startswith(p) for p in prefixes)]
        trainer = training.Trainer(None, None, update_vars=picked)
        trainer._alloc_grads(layer_vars, torch.device('cpu'))
        tables[name] = training._var_table(layer_vars, trainer.offsets, trainer.layer_ends)[0]
    h = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, 80, ctypes.byref(h)))      # no context: sizing only
    for dtype in range(5):
        _lib.check(L.y3_net_set_dtype(h, dtype))
        for side in (None, ctypes.c_void_p(0x1000)):
            _lib.check(L.y3_net_train_set_wgrad_stream(h, side))
            for size in (64, 256, 416, 608):
                for n in (1, 4, 64):
                    for name in sorted(tables):
                        print("dtype %d stream %s %dx%d bs %d %s: %d" % (dtype, 'on' if side else 'off', size, size, n, name,
                                                                         L.y3_net_train_workspace_bytes(h, tables[name], n, size, size)))
    _lib.check(L.y3_net_train_set_wgrad_stream(h, None))
    L.y3_net_destroy(h)


if __name__ == "__main__":
    main()
