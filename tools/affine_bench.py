"""Kernel time of y3_affine beside y3_mosaic on the same batch (profiles/affine_rate.txt).

    python tools/affine_bench.py [--batch 64] [--size 416] [--kmax 8,70] [--rounds 5] [--calls 20]

4 * batch samples of size x size are composed into `batch` images by utils.data_utils.mosaic_batch, and those images are
warped by utils.data_utils.affine_batch with records drawn at (10 degrees, 0.1, 0.5, 2 degrees).  Each entry point is timed
between device events around `calls` calls, `rounds` times over, the two alternating; the figure is the wrapper's call, as
the feeder makes it (record check, upload of the records, both kernels)."""
import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RANGES = (10.0, 0.1, 0.5, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--kmax', default='8,70', help="boxes per sample, every sample full")
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils.data_aug import affine_draw, mosaic_draw
    from yolov3_tensorflow_amd.utils.data_utils import affine_batch, mosaic_batch
    dev = fw.default_device()
    n, s = args.batch, args.size
    prng, rng = random.Random(1), np.random.RandomState(1)
    samples = torch.rand((4 * n, s, s, 3), dtype=torch.float32, device=dev)
    cuts = [mosaic_draw(prng, s, s) for _ in range(n)]
    warps = [affine_draw(prng, s, s, *RANGES) for _ in range(n)]
    image_mb = n * s * s * 3 * 4 / 1e6
    for kmax in [int(v) for v in args.kmax.split(',')]:
        x0, y0 = rng.uniform(0, 0.7 * s, (4 * n, kmax)), rng.uniform(0, 0.7 * s, (4 * n, kmax))
        b = np.stack([x0, y0, x0 + rng.uniform(8, 0.3 * s, x0.shape), y0 + rng.uniform(8, 0.3 * s, x0.shape), np.ones_like(x0)], axis=2)
        boxes = torch.from_numpy(b.astype(np.float32)).to(dev)
        labels = torch.from_numpy(rng.randint(0, 80, (4 * n, kmax)).astype(np.int32)).to(dev)
        counts = torch.full((4 * n,), kmax, dtype=torch.int32, device=dev)
        composed = mosaic_batch(samples, boxes, labels, counts, cuts)
        arms = {'y3_mosaic': lambda: mosaic_batch(samples, boxes, labels, counts, cuts),
                'y3_affine': lambda: affine_batch(*composed, warps)}
        kept = {'y3_mosaic': int(composed[3].sum()), 'y3_affine': int(arms['y3_affine']()[3].sum())}
        for fn in arms.values():        # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.calls):
                    fn()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) / args.calls)
        for name in arms:
            best = min(times[name])
            print('%s n=%d %dx%d kmax=%d: %s ms per call (%d x %d calls; kept %d boxes); %.0f MB read + written -> %.0f GB/s at '
                  'the best' % (name, n, s, s, kmax if name == 'y3_mosaic' else 4 * kmax, ' '.join('%.3f' % t for t in times[name]),
                                args.rounds, args.calls, kept[name], 2 * image_mb, 2 * image_mb / best), flush=True)


if __name__ == '__main__':
    main()
