"""Time the optimizer update alone on the full network's 222 trainable tensors (no forward, no backward).

    python tools/update_bench.py [--classes 80] [--rounds 5] [--calls 20] [--out profiles/layerwise_update_rate.txt]

Arms: momentum and adam through y3_clip_update_multi, adamw / lars / lamb through y3_layerwise_update_multi.  The arms
alternate in one process; each measurement is one pair of events around `calls` back-to-back calls, `rounds` times per arm.
Tensor sizes come from the library's own layer table (conv kernel, then BN gamma / beta or the bias, per layer).  Gradients
are re-used from call to call (the update scales and clips them in place, so they shrink towards the clip norm and stay
finite); the numbers are times, not a training run.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

ARMS = ('momentum', 'adam', 'adamw', 'lars', 'lamb')
# full passes over a tensor's elements per call, for the bytes column.  prepare: read g and w, write g (3).  update: read
# and write g, w and each slot (momentum, lars 6; adam, adamw 8).  lamb: direction reads g, w, m, v and writes g, m, v (7),
# apply reads g and w and writes w (3).
PASSES = dict(momentum=3 + 6, adam=3 + 8, adamw=3 + 8, lars=3 + 6, lamb=3 + 7 + 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from yolov3_tensorflow_amd import build, framework as fw, training, _lib
    build.build(verbose=False)
    L, ctx, dev = _lib.lib(), fw.context(), fw.default_device()
    sizes, kernel = [], []
    for l in training._Topology(a.classes).layers:
        sizes.append(l['k'] * l['k'] * l['cin'] * l['cout'])
        kernel.append(True)
        for _ in range(2 if l['bn'] else 1):
            sizes.append(l['cout'])
            kernel.append(False)
    count, total = len(sizes), int(sum(sizes))
    offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])]).astype(np.int64)
    gen = torch.Generator(device='cpu').manual_seed(0)
    flat = lambda scale: (torch.randn(int(offs[-1]), generator=gen) * scale).to(dev)
    w, g, s0, s1 = flat(0.05), flat(1e-3), flat(1e-3), flat(1e-3).abs_()
    arr = (_lib.ParamDesc * count)()
    for i, n in enumerate(sizes):
        p = lambda t: t.data_ptr() + 4 * int(offs[i])
        arr[i] = _lib.ParamDesc(p(w), p(g), p(s0), p(s1), n, 5e-4 if kernel[i] else 0.0, 0 if kernel[i] else _lib.Y3_PARAM_NO_ADAPT)
    nb = max(L.y3_clip_update_multi_scratch_bytes(arr, count), L.y3_layerwise_update_multi_scratch_bytes(arr, count))
    sc = torch.empty(nb, dtype=torch.uint8, device=dev)
    ratios = torch.empty(count, dtype=torch.float32, device=dev)
    cf = ctypes.c_float
    hp = _lib.LayerwiseHp(grad_scale=1.0, clip_norm=100.0, lr=1e-4, lr_t=1e-4, momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-6,
                          bias1=1.0, bias2=1.0, trust=1e-3, ema_step=0.0)

    def call(arm):
        if arm in ('momentum', 'adam'):
            _lib.check(L.y3_clip_update_multi(ctx, training.Optimizer.KINDS.index(arm), arr, count, cf(1.0), cf(100.0), cf(1e-4),
                                              cf(0.9), cf(0.9), cf(0.999), cf(1e-8), fw.ptr(sc), ctypes.c_size_t(nb)))
        else:
            _lib.check(L.y3_layerwise_update_multi(ctx, training.Optimizer.KINDS.index(arm), arr, count, ctypes.byref(hp), None,
                                                   fw.ptr(ratios), fw.ptr(sc), ctypes.c_size_t(nb)))

    for arm in ARMS:                    # warm-up: code objects, the pinned staging buffer
        call(arm)
    torch.cuda.synchronize()
    times = {arm: [] for arm in ARMS}
    for _ in range(a.rounds):
        for arm in ARMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call(arm)
            e1.record()
            e1.synchronize()
            times[arm].append(e0.elapsed_time(e1) / a.calls)
    fw.check_context()
    assert bool(torch.isfinite(w).all())
    lines = ['optimizer update alone: %d tensors, %d elements (%.1f MB fp32), %d x %d calls per arm, arms alternating'
             % (count, total, total * 4 / 1e6, a.rounds, a.calls),
             '%-9s %-28s %9s %9s %9s %8s %9s' % ('arm', 'entry', 'min ms', 'median', 'max ms', 'passes', 'GB/s(min)')]
    for arm in ARMS:
        t = sorted(times[arm])
        entry = 'y3_clip_update_multi' if arm in ('momentum', 'adam') else 'y3_layerwise_update_multi'
        lines.append('%-9s %-28s %9.4f %9.4f %9.4f %8d %9.0f' % (arm, entry, t[0], t[len(t) // 2], t[-1], PASSES[arm],
                                                                 PASSES[arm] * total * 4 / 1e9 / (t[0] * 1e-3)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
