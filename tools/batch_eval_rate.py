"""What one evaluation of the training batch costs, host path against eval_utils.evaluate_on_device, on one seeded synthetic
batch at the bench training configuration (bs 64, 416x416, 80 classes) with train.py's defaults (nms_topk 150, score
threshold 0.01, nms / iou threshold 0.45).  y_true holds about 7 objects per image; y_pred is [64, 10647, ...] with noisy
copies of the objects and clutter above the score threshold, everything else below it.  Both paths start from the same
device tensors:

  host      eval_utils.evaluate_on_gpu with functools.partial(gpu_nms, ...): y_pred and y_true to numpy, gpu_nms per image
  device    eval_utils.evaluate_on_device: gpu_nms_batched once, y3_batch_eval, one table back; the two parts also timed
            apart with events

Median of --reps runs after --warmup, torch.cuda.synchronize() around each; both results are compared.  Writes --out.

    python tools/batch_eval_rate.py [--batch 64] [--reps 10] [--warmup 2] [--out profiles/batch_eval_rate.txt]
"""
import argparse
import functools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES, SIZE, LIVE = 80, 416, 400


def synthetic(n, seed=0):
    """(y_pred, y_true) on the host: per image 3 .. 11 objects in random cells, LIVE boxes with a score above 0.01."""
    rng = np.random.RandomState(seed)
    grids = [SIZE // 32, SIZE // 16, SIZE // 8]
    B = sum(3 * g * g for g in grids)
    y_true = [np.zeros((n, g, g, 3, 5 + CLASSES + 1), np.float32) for g in grids]
    boxes = np.zeros((n, B, 4), np.float32)
    confs = np.full((n, B, 1), 1e-4, np.float32)
    probs = np.full((n, B, CLASSES), 1e-3, np.float32)
    xy = rng.uniform(0, SIZE - 40, (n, B, 2))
    boxes[:] = np.concatenate([xy, xy + rng.uniform(10, 120, (n, B, 2))], 2)
    for i in range(n):
        k = int(rng.randint(3, 12))
        wh = rng.uniform(20, 200, (k, 2))
        c = np.stack([rng.uniform(wh[:, 0] / 2, SIZE - wh[:, 0] / 2), rng.uniform(wh[:, 1] / 2, SIZE - wh[:, 1] / 2)], 1)
        labels = rng.randint(0, CLASSES, k)
        for j in range(k):
            s = int(rng.randint(0, 3))
            cell = y_true[s][i, int(rng.randint(0, grids[s])), int(rng.randint(0, grids[s])), int(rng.randint(0, 3))]
            cell[0:2], cell[2:4], cell[4], cell[5 + labels[j]], cell[-1] = c[j], wh[j], 1., 1., 1.
        live = rng.permutation(B)[:LIVE]
        near = rng.randint(0, k, LIVE // 2)
        gt = np.concatenate([c - wh / 2, c + wh / 2], 1)
        boxes[i, live[:LIVE // 2]] = gt[near] + rng.normal(0, 5.0, (LIVE // 2, 4))
        lab = np.concatenate([labels[near], rng.randint(0, CLASSES, LIVE - LIVE // 2)])
        confs[i, live, 0] = rng.uniform(0.2, 1.0, LIVE)
        probs[i, live, lab] = rng.uniform(0.3, 1.0, LIVE)
    return (boxes, confs, probs), y_true


def median_ms(fn, reps, warmup):
    import torch
    times = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_eval_rate.txt'))
    args = ap.parse_args(argv)
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils import eval_utils
    from yolov3_tensorflow_amd.utils.nms_utils import gpu_nms, gpu_nms_batched
    dev = fw.default_device()
    topk, score, nms = 150, 0.01, 0.45
    y_pred, y_true = synthetic(args.batch)
    y_pred = tuple(torch.from_numpy(a).to(dev) for a in y_pred)
    y_true = [torch.from_numpy(a).to(dev) for a in y_true]
    op = functools.partial(gpu_nms, num_classes=CLASSES, max_boxes=topk, score_thresh=score, nms_thresh=nms)
    host = lambda: eval_utils.evaluate_on_gpu(None, op, None, None, y_pred, y_true, CLASSES, nms)
    device = lambda: eval_utils.evaluate_on_device(y_pred, y_true, CLASSES, topk, score, nms, iou_thresh=nms)
    t_dev, got = median_ms(device, args.reps, args.warmup)
    t_host, want = median_ms(host, args.reps, args.warmup)

    def parts():      # the device path's two parts by events: scores + NMS, then y3_batch_eval
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        dets = gpu_nms_batched(y_pred[0], y_pred[1] * y_pred[2], CLASSES, topk, score, nms, lazy=True)
        ev[1].record()
        eval_utils.batch_eval_counts(dets, y_true, CLASSES, nms)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
    split = np.array([parts() for _ in range(args.warmup + args.reps)][args.warmup:])
    t_nms, t_eval = float(np.median(split[:, 0])), float(np.median(split[:, 1]))
    dets = gpu_nms_batched(y_pred[0], y_pred[1] * y_pred[2], CLASSES, topk, score, nms, lazy=True)
    n_det = int(dets.device_tensors()[3].sum().item())
    same = np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes() and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes()
    lines = ['batch_eval_rate: one training batch of %d images, %dx%d, %d classes; nms_topk %d, score threshold %g, nms / iou threshold %g; '
             '%d detections after NMS; median of %d after %d warm-ups' % (args.batch, SIZE, SIZE, CLASSES, topk, score, nms, n_det,
                                                                          args.reps, args.warmup),
             'host   (evaluate_on_gpu, gpu_nms per image, numpy matching): %.2f ms' % t_host,
             'device (evaluate_on_device): %.3f ms wall, of which by events: scores + gpu_nms_batched %.3f ms, y3_batch_eval %.3f ms'
             % (t_dev, t_nms, t_eval),
             'recall %.6f precision %.6f; host and device results bit-identical: %s' % (got[0], got[1], same)]
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
