#!/usr/bin/env python
"""Standalone throughput of the feeder: images/s decoded, augmented, resized and copied to the device with nothing
consuming them but this loop - how far the host side is from what the train step asks for (704 images/s per GPU at
416x416, bs=64: profiles/r03_bench_c4_n1.json).  Synthetic 640x480 JPEGs (COCO's usual size), 'train' mode with mix-up,
multi-scale off, batch 64.

    python tools/feeder_rate.py [--workers 8,16,32] [--backends thread,process] [--native 1,0] [--batches 12]
    python tools/feeder_rate.py --feeders 8 [--workers 10] [--backends thread]     # the host side of an 8-GPU node:
        eight feeder PROCESSES (one per rank, as train.py runs them) at once on this host, aggregate images/s against
        the 8 x 697 images/s eight train steps consume (VERDICT r3 #5b; every process uploads to cuda:0 here)
"""
import argparse
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = np.array([10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326], np.float32)
AFFINE = (10.0, 0.1, 0.5, 2.0)      # --affine 1: degrees, translate, scale, shear


def write_set(folder, n, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        w, h = 640, 480
        small = rng.randint(0, 256, (h // 10, w // 10, 3)).astype(np.uint8)
        path = str(folder / ('img_%d.jpg' % i))
        Image.fromarray(small).resize((w, h), Image.BICUBIC).save(path, quality=90)
        parts = ['%d' % i, path, '%d' % w, '%d' % h]
        for _ in range(int(rng.randint(1, 8))):
            x0, y0 = rng.uniform(0, w * 0.5), rng.uniform(0, h * 0.5)
            parts += ['%d' % rng.randint(0, 80), '%.1f' % x0, '%.1f' % y0, '%.1f' % (x0 + rng.uniform(20, w * 0.45)),
                      '%.1f' % (y0 + rng.uniform(20, h * 0.45))]
        lines.append(' '.join(parts))
    return lines


def timed_batches(it, batches, sync=lambda: None, meet=lambda: None):
    """Three batches of warm-up (pool start-up, pinned buffers), then `batches` on the clock: (start, end, CPU seconds)."""
    for _ in range(3):
        next(it)
    sync()
    meet()
    t0, c0 = time.time(), time.process_time()
    for _ in range(batches):
        next(it)
    sync()
    return t0, time.time(), time.process_time() - c0


def host_half(f):
    """The feeder's host half alone (decode, augmentation chain, resize into a float32 batch buffer, collate): nothing is
    uploaded or launched, so eight of these on a one-GPU box measure the HOST of an eight-GPU node (with uploads, eight
    processes time-slice the one device here and the figure is the slicing, not the host)."""
    import threading
    from yolov3_tensorflow_amd import feeder as fd
    shared = fd._SharedBuffers()
    try:
        for batch in f._host_batches(0, f._delivery(fd._Buffers(), shared), threading.Event()):
            if batch[-1] is not None:       # recycled at once, as the feeder's buffers are after their upload
                batch[-1][0].give(None, batch[-1][1])
            yield batch
    finally:
        shared.close()


def _one_feeder(rank, nfeed, lines, args, backend, workers, barrier, out):
    """One rank's feeder in its own process: warm up, meet the others, serve `batches` batches, report the window."""
    import torch
    from yolov3_tensorflow_amd.feeder import Feeder
    try:
        f = Feeder(lines, args.batch_size, 80, [416, 416], ANCHORS, mode='train', use_mix_up=True, num_threads=workers,
                   prefetch=5, seed=1 + rank, backend=backend, pixels=args.pixels.split(',')[0])
        it, sync = (host_half(f), lambda: None) if args.host_only else (f.epoch(0), torch.cuda.synchronize)
        t0, t1, cpu = timed_batches(it, args.batches, sync, lambda: barrier.wait(timeout=180))
        out.put((rank, t0, t1, None, cpu))
        it.close()
        f.close()
    except BaseException as e:      # noqa: BLE001 - reported by the parent; never leave the others at the barrier
        barrier.abort()
        out.put((rank, 0.0, 0.0, '%s: %s' % (type(e).__name__, e)))


def concurrent_feeders(args, lines):
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    n = args.feeders
    for backend in args.backends.split(','):
        for workers in [int(v) for v in args.workers.split(',')]:
            barrier, out = ctx.Barrier(n), ctx.Queue()
            procs = [ctx.Process(target=_one_feeder, args=(r, n, lines, args, backend, workers, barrier, out)) for r in range(n)]
            for p in procs:
                p.start()
            res = []
            try:
                for _ in range(n):
                    res.append(out.get(timeout=420))
            except Exception:       # noqa: BLE001 - queue.Empty: a feeder never reported
                pass
            for p in procs:
                p.join(timeout=20)
                if p.is_alive():
                    p.terminate()
            bad = [r for r in res if r[3]]
            if len(res) < n or bad:
                print('%d feeders, backend=%s, %d workers: FAILED (%d reports; %s)' % (n, backend, workers, len(res),
                                                                                      '; '.join(str(r[3]) for r in bad)), flush=True)
                continue
            span = max(r[2] for r in res) - min(r[1] for r in res)
            per = [args.batches * args.batch_size / (r[2] - r[1]) for r in res]
            total = n * args.batches * args.batch_size / span
            cpu = [r[4] for r in res if len(r) > 4]
            print('%d feeders at once%s, pixels=%s, backend=%s, %d workers each: aggregate %.0f images/s (per feeder min %.0f / mean %.0f / '
                  'max %.0f) against %d x 697 = %d images/s consumed by %d train steps: %.2fx%s'
                  % (n, ' (host half only)' if args.host_only else '', args.pixels.split(',')[0], backend, workers, total, min(per),
                     sum(per) / n, max(per), n, n * 697, n, total / (n * 697.0),
                     '; %.2f ms of CPU per image' % (1e3 * sum(cpu) / (n * args.batches * args.batch_size)) if cpu else ''), flush=True)


def timed_epochs(f, args, label):
    """Whole epochs over the same files, each timed on its own (epoch 0 after 3 warm-up batches)."""
    import torch
    for epoch in range(args.epochs):
        it = f.epoch(epoch)
        images = 0
        if epoch == 0:
            for _ in range(3):
                next(it)
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        for b in it:
            images += len(b.image_ids)
        torch.cuda.synchronize()
        dt, cpu = time.perf_counter() - t0, time.process_time() - c0
        stats = (' cache %r' % (f.cache.stats(),)) if f.cache is not None else ''
        print('%s epoch %d: %5d images %7.0f images/s, %.2f ms of this process\'s CPU per image%s' % (
            label, epoch, images, images / dt, 1e3 * cpu / images, stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host-only', action='store_true', help="with --feeders: the host half only (no upload, no device)")
    ap.add_argument('--feeders', type=int, default=0, help="run this many feeder processes concurrently (one per rank of a node)")
    ap.add_argument('--workers', default='8,16,32')
    ap.add_argument('--backends', default='thread,process')
    ap.add_argument('--native', default='1,0')
    ap.add_argument('--pixels', default='host', help="host,gpu: where the pixel work runs (Feeder(pixels=...); thread backend, "
                                                     "native=1 for gpu); with --feeders the first entry is used")
    ap.add_argument('--batches', type=int, default=12)
    ap.add_argument('--cache_gb', type=float, default=0, help="Feeder(cache_bytes=...): keep decoded sources on the device "
                                                                "(pixels=gpu only)")
    ap.add_argument('--epochs', type=int, default=1, help="time this many epochs over the SAME files (the first 3 batches of "
                                                           "epoch 0 are warm-up): with --cache_gb, epochs 1.. are cached ones")
    ap.add_argument('--batch_size', type=int, default=64)
    ap.add_argument('--mosaic', default='0', help="0,1: Feeder(mosaic=...) - four samples composed into every image on the "
                                                  "device; both values in one call give the pair of rates")
    ap.add_argument('--affine', default='0', help="0,1: Feeder(affine=(10, 0.1, 0.5, 2)) - every delivered image warped on the "
                                                  "device; both values in one call give the pair of rates")
    ap.add_argument('--repeat', type=int, default=1, help="run the --mosaic / --affine arms this many times over, alternating")
    ap.add_argument('--check', action='store_true', help="first compare the first batch of a process-backed feeder with a "
                                                         "thread-backed one (same seed): they must be equal")
    args = ap.parse_args()
    import torch
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = write_set(pathlib.Path(tempfile.mkdtemp()), 256)
    if args.epochs > 1:          # an epoch is the 256 files once (more, distinct, when --batches asks for more)
        lines = write_set(pathlib.Path(tempfile.mkdtemp()), max(256, args.batches * args.batch_size))
    else:
        lines = (lines * ((args.batches + 9) * args.batch_size // len(lines) + 1))[:(args.batches + 9) * args.batch_size]
    print('host threads available: %d' % len(os.sched_getaffinity(0)), flush=True)
    if args.feeders > 0:
        concurrent_feeders(args, lines)
        return
    if args.check:
        first = {}
        for backend in ('thread', 'process'):
            f = Feeder(lines[:32], 16, 80, [416, 416], ANCHORS, mode='train', use_mix_up=True, num_threads=4, prefetch=2,
                       seed=5, backend=backend)
            it = f.epoch(0)
            b = next(it)
            torch.cuda.synchronize()
            first[backend] = [b.images.cpu()] + [y.cpu() for y in b.y_true]
            it.close()
            f.close()
        same = all(torch.equal(x, y) for x, y in zip(first['thread'], first['process']))
        print('first batch: process-backed feeder %s thread-backed feeder' % ('==' if same else '!='), flush=True)
    for native in args.native.split(','):
        os.environ['Y3_FEED_NATIVE'] = native
        for backend in args.backends.split(','):
            for workers in [int(v) for v in args.workers.split(',')]:
                for pixels in args.pixels.split(','):
                    if pixels == 'gpu' and (backend != 'thread' or native != '1'):
                        continue
                    cache = int(args.cache_gb * (1 << 30)) if pixels == 'gpu' else 0
                    arms = [(m == '1', a == '1') for m in args.mosaic.split(',') for a in args.affine.split(',')]
                    for mosaic, affine in arms * args.repeat:
                        f = Feeder(lines, args.batch_size, 80, [416, 416], ANCHORS, mode='train', use_mix_up=True,
                                   num_threads=workers, prefetch=5, seed=1, backend=backend, pixels=pixels, cache_bytes=cache,
                                   mosaic=mosaic, affine=AFFINE if affine else None)
                        if args.epochs > 1:
                            timed_epochs(f, args, 'native=%s backend=%-7s workers=%3d pixels=%-4s cache=%gGB mosaic=%d affine=%d' % (
                                native, backend, workers, pixels, args.cache_gb if cache else 0, mosaic, affine))
                            f.close()
                            continue
                        it = f.epoch(0)
                        t0, t1, cpu = timed_batches(it, args.batches, torch.cuda.synchronize)
                        dt = t1 - t0
                        it.close()
                        f.close()
                        images = args.batches * args.batch_size
                        print('native=%s backend=%-7s workers=%3d pixels=%-4s mosaic=%d affine=%d: %7.0f images/s%s' % (
                            native, backend, workers, pixels, mosaic, affine, images / dt,
                            ', %.2f ms of this process\'s CPU per image' % (1e3 * cpu / images) if backend == 'thread' else ''),
                            flush=True)


if __name__ == '__main__':
    main()
