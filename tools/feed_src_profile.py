#!/usr/bin/env python
"""One training-size batch (64 jobs, 640x480 sources, mix-up, expansion, letterbox to 416x416) a few times through one leg,
for a kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/feed_src_profile.py --leg LEG [--repeat 20]

    packed  every source packed into the batch's blob (what a feeder without a source cache runs)
    arena   every source in a device arena, read there by reference

Both go through y3_feed_run (feed_window_kernel<false> / <true>, feed_horizontal_kernel, feed_output_kernel).  Every leg first
computes the packed result in its own process and ends by comparing its bytes with it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('packed', 'arena'), required=True)
    ap.add_argument('--repeat', type=int, default=20)
    args = ap.parse_args()
    import torch
    from yolov3_tensorflow_amd import feed_native as fn
    from yolov3_tensorflow_amd.feed_cache import SourceCache
    from yolov3_tensorflow_amd.feed_device import DevicePixels
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (48, 64, 3)).astype(np.uint8).repeat(10, 0).repeat(10, 1) for _ in range(64)]
    packed, keyed = [], []
    for i in range(64):
        partner = (i + 1) % 64 if i % 2 else None
        ratio = rng.uniform(1, 4) if i % 2 else 1.0
        cw, ch = int(640 * ratio), int(480 * ratio)
        off = (int(rng.randint(0, cw - 640 + 1)), int(rng.randint(0, ch - 480 + 1)))
        ww, wh = int(rng.randint(cw // 3, cw + 1)), int(rng.randint(ch // 3, ch + 1))
        window = (int(rng.randint(0, cw - ww + 1)), int(rng.randint(0, ch - wh + 1)), ww, wh)
        scale = min(416 / ww, 416 / wh)
        resized = (max(1, int(ww * scale)), max(1, int(wh * scale)))
        kw = dict(lam=float(rng.beta(1.5, 1.5)) if partner is not None else 1.0,
                  colour=(int(rng.randint(-32, 33)), int(rng.randint(-18, 19)), float(rng.uniform(0.5, 1.5)),
                          float(rng.uniform(0.5, 1.5))),
                  offset=off, window=window, interp=i % 5, resized=resized, out_size=(416, 416),
                  pad=((416 - resized[0]) // 2, (416 - resized[1]) // 2), pad_value=128, flip_x=bool(i % 2))
        for jobs in (packed, keyed):
            pj = fn.make_job(images[i], None if partner is None else images[partner], **kw)
            jobs.append(pj)
        keyed[-1].key1, keyed[-1].key2 = i, partner
    dp = DevicePixels()
    want = dp.run(packed)
    cache = SourceCache(dp.device, 64 * 480 * 640 * 3 + 4096) if args.leg == 'arena' else None
    jobs = packed if cache is None else keyed
    got = dp.run(jobs, cache=cache)             # (arena: takes every image in)
    for _ in range(args.repeat):
        got = dp.run(jobs, cache=cache)
    torch.cuda.synchronize()
    if cache is not None:
        print('cache: %r' % (cache.stats(),))
        assert cache.stats()['images'] == 64, cache.stats()
    same = bool(torch.equal(want, got))
    print('%s == packed: %s' % (args.leg, same))
    assert same


if __name__ == '__main__':
    main()
