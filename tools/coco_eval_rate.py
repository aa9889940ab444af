"""What the COCO metrics cost behind the last kernel, host path against eval_utils.DeviceEval.finish_coco, on the seeded
synthetic set of tools/eval_rate.py (5,000 images, 80 classes, about 7 objects per image, 100 detections per image: half
jittered ground truth, half clutter; scores distinct).  Both paths start from the same NMS-shaped device tensors (batches of 32):

  host      eval_utils.get_preds_batch per batch (device -> host, one Python row per detection), then eval_utils.coco_eval
  device    DeviceEval.add per batch, then DeviceEval.finish_coco (stats and per_class back); for comparison DeviceEval.finish
            (PASCAL VOC, one threshold) on the same arena

Every time is wall time with the stream drained before the clock starts and before it stops; the median of --runs runs (at
least 5) after one warm-up run.  The device numbers are compared with the host's (precision and recall equal, the twelve
numbers within n * 2**-52).  Writes the lines to --out.

    python tools/coco_eval_rate.py [--images 5000] [--dets 100] [--runs 5] [--out profiles/coco_eval_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from eval_rate import synthetic, CLASSES, BATCH      # noqa: E402


def median_time(fn, runs, sync, warmup=1):
    out, times = None, []
    for i in range(warmup + runs):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times)), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_eval_rate.txt'))
    args = ap.parse_args(argv)
    if args.runs < 5:
        ap.error('--runs must be at least 5')
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils import eval_utils
    dev = fw.default_device()
    sync = torch.cuda.synchronize
    dets = args.dets
    gt_dict, batches = synthetic(args.images, dets)
    on_dev = [(ids,) + tuple(torch.from_numpy(x).to(dev) for x in rest) for ids, *rest in batches]
    lines = ['coco_eval_rate: %d images, %d classes, %d detections per image (%d rows), batches of %d; wall time, stream drained, '
             'median (min .. max) of %d runs after 1 warm-up' % (args.images, CLASSES, dets, args.images * dets, BATCH, args.runs)]

    def filled():
        ev = eval_utils.DeviceEval(gt_dict, list(gt_dict), CLASSES, capacity_rows=args.images * dets)
        for ids, ob, osc, ol, cnt in on_dev:
            ev.add(ids, (ob, osc, ol, cnt))
        return ev
    ev = filled()
    t_add = median_time(lambda: filled(), args.runs, sync)[:3]
    t_coco = median_time(lambda: ev.finish_coco(return_curves=True), args.runs, sync)
    got = t_coco[3]
    t_coco_short = median_time(lambda: ev.finish_coco(), args.runs, sync)[:3]
    t_voc = median_time(lambda: ev.finish(), args.runs, sync)[:3]

    def rows():
        out = []
        for ids, ob, osc, ol, cnt in on_dev:
            out.extend(eval_utils.get_preds_batch(ids, [(ob[i, :dets], osc[i, :dets], ol[i, :dets]) for i in range(len(ids))]))
        return out
    t_rows = median_time(rows, args.runs, sync, warmup=0)
    val_preds = t_rows[3]
    t_host = median_time(lambda: eval_utils.coco_eval(gt_dict, val_preds, CLASSES), args.runs, sync, warmup=0)
    want = t_host[3]
    same = bool(np.array_equal(got['precision'], want['precision']) and np.array_equal(got['recall'], want['recall']))
    gap = float(np.abs(got['stats'] - want['stats']).max())
    fmt = lambda t, unit=1.: '%.3f (%.3f .. %.3f)' % (t[0] * unit, t[1] * unit, t[2] * unit)
    lines += ['host   get_preds_batch (rows to Python)            %s s' % fmt(t_rows),
              'host   coco_eval                                   %s s' % fmt(t_host),
              'device DeviceEval construction + %4d x add         %s ms' % (len(on_dev), fmt(t_add, 1e3)),
              'device finish_coco (stats, per_class back)         %s ms' % fmt(t_coco_short, 1e3),
              'device finish_coco(return_curves=True)             %s ms' % fmt(t_coco, 1e3),
              'device finish (PASCAL VOC, same arena)             %s ms' % fmt(t_voc, 1e3),
              'precision and recall equal to coco_eval: %s   max |stats gap| = %.3g (bound n * 2.2e-16)   AP %.4f AP50 %.4f AR100 %.4f'
              % (same, gap, got['stats'][0], got['stats'][1], got['stats'][8])]
    for line in lines:
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
