"""Kernel times of y3_spp_fwd / y3_spp_bwd next to their byte floors, and the SPP architecture's inference forward beside the
default architecture's (profiles/spp_rate.txt).

    python tools/spp_bench.py [--rounds 5] [--calls 20] [--rate 5.0] [--no-forward]

The pool launches at the shapes of the workloads: bs = 32 @416 fp32 and bs = 16 @608 bf16 (inference: forward only), bs = 64
@416 in fp32 and bf16 (training: forward, and backward in its overwriting form, reading x out of the materialised spp(x)).  Each entry point is timed
between device events around `calls` calls, `rounds` times over.  Floors: forward reads c and writes 4c per position,
backward reads x, reads 4c of g and writes c; at `rate` TB/s, the streaming rate DESIGN.md 4 measures for the BN passes.
The train step's times come from tools/train_bench.py [--spp]."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C = 512
CASES = [  # name, n, grid, bf16, backward too
    ('bs=32 @416 fp32', 32, 13, False, False), ('bs=16 @608 bf16', 16, 19, True, False),
    ('bs=64 @416 fp32 train', 64, 13, False, True), ('bs=64 @416 bf16 train', 64, 13, True, True)]


def timed(fn, rounds, calls):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rate', type=float, default=5.0, help='TB/s of the byte floors')
    ap.add_argument('--no-forward', action='store_true')
    a = ap.parse_args()
    import torch
    from yolov3_tensorflow_amd import engine, framework as fw
    dev = fw.default_device()
    for name, n, g, bf16, bwd in CASES:
        dt, es = (torch.bfloat16, 2) if bf16 else (torch.float32, 4)
        x = torch.randn((n, g, g, C), device=dev).to(dt)
        pos = n * g * g
        t = timed(lambda: engine.spp_fwd(x), a.rounds, a.calls)
        floor = pos * 5 * C * es / (a.rate * 1e12) * 1e3
        print('y3_spp_fwd %s [%d,%d,%d,%d]: %s ms per call; floor %.4f ms (%.1f MB at %.1f TB/s); best = %.1f x floor'
              % (name, n, g, g, C, ' '.join('%.4f' % v for v in t), floor, pos * 5 * C * es / 1e6, a.rate, min(t) / floor), flush=True)
        if not bwd:
            continue
        pooled = engine.spp_fwd(x)
        grad = torch.randn((n, g, g, 4 * C), device=dev)
        t = timed(lambda: engine.spp_bwd(pooled[..., 3 * C:], grad, x_stride=4 * C), a.rounds, a.calls)      # (overwrites dx)
        nbytes = pos * C * (es + 16 + 4)                # x, 4c of g, dx written
        floor = nbytes / (a.rate * 1e12) * 1e3
        print('y3_spp_bwd %s [%d,%d,%d,%d]: %s ms per call; floor %.4f ms (%.1f MB at %.1f TB/s); best = %.1f x floor'
              % (name, n, g, g, C, ' '.join('%.4f' % v for v in t), floor, nbytes / 1e6, a.rate, min(t) / floor), flush=True)
    if a.no_forward:
        return
    import yolov3_tensorflow_amd as y3
    import bench
    for n, size, dtype in ((32, 416, 'f32_wino'), (16, 608, 'bf16')):
        xs = torch.rand((n, size, size, 3), device=dev)
        for spp in (False, True):
            y3.reset_default_graph()
            model = y3.yolov3(80, bench.ANCHORS)
            model.compute_dtype, model.spp = dtype, spp
            with y3.variable_scope('yolov3'):
                model.forward(torch.zeros((1, 64, 64, 3), device=dev))
                bench.random_init(1)
                t = timed(lambda: model.forward(xs, False), a.rounds, max(a.calls // 4, 2))
                ms, table = model.layer_times_ms(xs, iters=4)
            line = 'forward %s bs=%d @%d, %s: %s ms' % ('SPP    ' if spp else 'default', n, size, dtype, ' '.join('%.3f' % v for v in t))
            if spp:
                line += '; layer 55 (pool + 1x1 2048->512) %.4f ms, layer 54 (1x1 1024->512) %.4f ms' % (ms[55], ms[54])
            print(line, flush=True)


if __name__ == '__main__':
    main()
