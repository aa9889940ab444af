#!/usr/bin/env python
"""One training-size batch (64 jobs, 640x480 sources, mix-up, expansion, letterbox to 416x416) through y3_feed_run (packed
sources) and through y3_feed_run_src (every source in a device arena), a few times each, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/feed_src_profile.py [--repeat 20]

The three kernels of either entry show up under their own names (feed_*_kernel / feed_*_src_kernel).  The two results
are compared before the script ends."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    args = ap.parse_args()
    import torch
    from yolov3_tensorflow_amd import feed_native as fn
    from yolov3_tensorflow_amd.feed_cache import SourceCache
    from yolov3_tensorflow_amd.feed_device import DevicePixels
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (48, 64, 3)).astype(np.uint8).repeat(10, 0).repeat(10, 1) for _ in range(64)]
    packed, by_ref = [], []
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
        for jobs in (packed, by_ref):
            pj = fn.make_job(images[i], None if partner is None else images[partner], **kw)
            pj.key1, pj.key2 = i, partner
            jobs.append(pj)
    dp = DevicePixels()
    cache = SourceCache(dp.device, 64 * 480 * 640 * 3 + 4096)
    want = dp.run(packed)
    got = dp.run(by_ref, cache=cache)           # (takes every image in)
    for _ in range(args.repeat):
        want = dp.run(packed)
        got = dp.run(by_ref, cache=cache)
    torch.cuda.synchronize()
    print('cache: %r' % (cache.stats(),))
    print('y3_feed_run_src == y3_feed_run: %s' % bool(torch.equal(want, got)))


if __name__ == '__main__':
    main()
