"""What the mAP bookkeeping behind the last kernel costs, host path against eval_utils.DeviceEval, on one seeded synthetic
set (5,000 images, 80 classes, about 7 objects per image, 100 and 400 detections per image: half jittered ground truth, half
clutter; scores distinct).  Both paths start from the same NMS-shaped device tensors (boxes [32,cap,4], scores, labels,
counts per batch of 32):

  host      eval_utils.get_preds_batch per batch (device -> host, one Python row per detection), then voc_eval once per class
  device    DeviceEval.add per batch, then DeviceEval.finish (one [80, 5] table back); wall time with the stream drained

and both tables are compared (npos, nd, recall, precision equal; area AP within nd * 2**-52).  Writes the times to --out.

    python tools/eval_rate.py [--images 5000] [--dets 100 400] [--out profiles/eval_map_rate.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES, BATCH = 80, 32


def synthetic(images, dets, seed=0):
    """gt_dict and, per batch, (ids, boxes [n,dets,4] f32, scores [n,dets] f32, labels [n,dets] i32, counts [n] i32)."""
    rng = np.random.RandomState(seed)
    gt_dict, batches = {}, []
    scores = (0.01 + (rng.permutation(images * dets) + 0.5) * (0.98 / (images * dets))).astype(np.float32)
    assert len(np.unique(scores)) == scores.size
    scores = scores.reshape(images, dets)
    for b0 in range(0, images, BATCH):
        ids = list(range(b0, min(b0 + BATCH, images)))
        ob, ol = np.empty((len(ids), dets, 4), np.float32), np.empty((len(ids), dets), np.int32)
        for i, img in enumerate(ids):
            k = int(rng.randint(3, 12))
            xy = rng.uniform(0, 300, (k, 2))
            g = np.concatenate([xy, xy + rng.uniform(10, 110, (k, 2))], 1)
            gl = rng.randint(0, CLASSES, k)
            gt_dict[img] = [[float(g[j, 0]), float(g[j, 1]), float(g[j, 2]), float(g[j, 3]), int(gl[j])] for j in range(k)]
            near = rng.randint(0, k, dets // 2)
            xy = rng.uniform(0, 300, (dets - dets // 2, 2))
            ob[i] = np.concatenate([g[near] + rng.normal(0, 5.0, (dets // 2, 4)),
                                    np.concatenate([xy, xy + rng.uniform(10, 110, xy.shape)], 1)])
            ol[i] = np.concatenate([gl[near], rng.randint(0, CLASSES, dets - dets // 2)])
        batches.append((ids, ob, scores[ids[0]:ids[-1] + 1].copy(), ol, np.full(len(ids), dets, np.int32)))
    return gt_dict, batches


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--dets', type=int, nargs='*', default=[100, 400])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_map_rate.txt'))
    args = ap.parse_args(argv)
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils import eval_utils
    dev = fw.default_device()
    lines = ['eval_rate: %d images, %d classes, batches of %d; host = get_preds_batch + %d x voc_eval, device = DeviceEval.add + finish'
             % (args.images, CLASSES, BATCH, CLASSES)]
    for dets in args.dets:
        gt_dict, batches = synthetic(args.images, dets)
        on_dev = [(ids,) + tuple(torch.from_numpy(x).to(dev) for x in rest) for ids, *rest in batches]
        # device: one warm-up pass (allocations, the sort's workspace), then the timed one
        for timed in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = eval_utils.DeviceEval(gt_dict, list(gt_dict), CLASSES, capacity_rows=args.images * dets)
            t1 = time.perf_counter()
            for ids, ob, osc, ol, cnt in on_dev:
                ev.add(ids, (ob, osc, ol, cnt))
            table = ev.finish()
            torch.cuda.synchronize()
            t_dev, t_setup = time.perf_counter() - t1, t1 - t0
        # host: the rows, then voc_eval per class
        t0 = time.perf_counter()
        val_preds = []
        for ids, ob, osc, ol, cnt in on_dev:
            val_preds.extend(eval_utils.get_preds_batch(ids, [(ob[i, :dets], osc[i, :dets], ol[i, :dets]) for i in range(len(ids))]))
        t_rows = time.perf_counter() - t0
        with np.errstate(all='ignore'), contextlib.redirect_stdout(io.StringIO()):
            want = np.array([[float(v) for v in eval_utils.voc_eval(gt_dict, val_preds, c)] for c in range(CLASSES)])
        t_host = time.perf_counter() - t0
        same = np.array_equal(table[:, :4], want[:, :4], equal_nan=True)
        ap_gap = float(np.nanmax(np.abs(table[:, 4] - want[:, 4]) / np.maximum(want[:, 1], 1.)))
        lines.append('%4d detections/image (%d rows): host %.2f s (rows %.2f s + voc_eval %.2f s)   device %.3f s (+ %.3f s one-off '
                     'ground-truth upload)   npos/nd/recall/precision equal: %s   max |AP gap| / nd = %.2g (bound 2.2e-16)   mAP %.4f'
                     % (dets, len(val_preds), t_host, t_rows, t_host - t_rows, t_dev, t_setup, same, ap_gap, float(table[:, 4].mean())))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
