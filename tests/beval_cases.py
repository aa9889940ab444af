"""Seeded cases for the training-batch evaluator (y3_batch_eval, include/yolo355.h): a y_true triple with objects written
straight into chosen cells, and detections in the layout y3_nms leaves them in (boxes [n,cap,4] f32, labels [n,cap] i32,
counts [n] i32) with poison in the slots past each image's count.  The expected value of every case is
eval_utils._evaluate itself, fed the prepared detections through an `nms_fn`, so no NMS runs on the CPU.
Shared by tests/test_batch_eval_cpu.py (the host build of csrc/y3_beval_px.h) and tests/test_batch_eval_gpu.py (the kernels).

Labels: L0 = 0, L1 = 1 % C, L2 = C - 1 (the class next to the mix-up channel).  With C = 1 the cases that need two labels
degenerate to one label; they are still compared with _evaluate, only their separating property is not asserted."""
import collections

import numpy as np

Case = collections.namedtuple('Case', 'name class_num h w y_true boxes labels counts iou_thresh gt_cap dropped expect')
# gt_cap: None = every cell of an image; dropped: the overflow word y3_batch_eval must report (0: the table is valid);
# expect: (sum n_tp, sum n_true, sum n_pred) the case was built to give when C > 1, or None


def grids(h, w):
    return [(h // 32, w // 32), (h // 16, w // 16), (h // 8, w // 8)]


def cells_of_image(h, w):
    return sum(3 * gh * gw for gh, gw in grids(h, w))


def empty_y_true(n, h, w, C):
    return [np.zeros((n, gh, gw, 3, 5 + C + 1), np.float32) for gh, gw in grids(h, w)]


def put(y_true, i, scale, row, col, anchor, xywh, classes, mix=1.0):
    """An object in cell (row, col, anchor) of `scale` of image i: classes = {class: entry of the class slice}."""
    cell = y_true[scale][i, row, col, anchor]
    assert not cell.any(), 'cell used twice'
    cell[0:4] = xywh
    cell[4] = 1.
    for c, v in classes.items():
        cell[5 + c] = v
    cell[-1] = mix


def corners(xywh, jitter=(0., 0., 0., 0.)):
    x, y, w, h = (float(np.float32(v)) for v in xywh)
    return [x - w / 2. + jitter[0], y - h / 2. + jitter[1], x + w / 2. + jitter[2], y + h / 2. + jitter[3]]


def pack(dets, pad=3):
    """dets: per image a list of ([x0, y0, x1, y1], label).  Slots past an image's count alternate between a NaN box of
    label 0 and a copy of the image's first detection: either would change the counts if it were read."""
    n = len(dets)
    cap = max(len(d) for d in dets) + pad
    boxes, labels, counts = np.full((n, cap, 4), np.nan, np.float32), np.zeros((n, cap), np.int32), np.zeros(n, np.int32)
    for i, d in enumerate(dets):
        counts[i] = len(d)
        for k, (b, l) in enumerate(d):
            boxes[i, k], labels[i, k] = np.asarray(b, np.float32), l
        for k in range(len(d) + 1, cap, 2):
            if d:
                boxes[i, k], labels[i, k] = boxes[i, 0], labels[i, 0]
    return boxes, labels, counts


def nms_fn_of(case):
    """The `nms_fn` _evaluate calls per image: the image index travels in boxes[0, 0, 0] of y_pred_of(case)."""
    def nms_fn(boxes, scores):
        i = int(boxes[0, 0, 0])
        k = int(case.counts[i])
        return case.boxes[i, :k].copy(), None, case.labels[i, :k].copy()
    return nms_fn


def y_pred_of(case):
    n = len(case.counts)
    return (np.arange(n, dtype=np.float32).reshape(n, 1, 1), np.ones((n, 1, 1), np.float32), np.ones((n, 1, 1), np.float32))


def reference_table(case, iou_thresh=None):
    """int64 [C, 3] = (n_tp, n_true, n_pred) from eval_utils._evaluate."""
    from yolov3_tensorflow_amd.utils import eval_utils
    thr = case.iou_thresh if iou_thresh is None else iou_thresh
    tp, true, pred = eval_utils._evaluate(y_pred_of(case), case.y_true, case.class_num, nms_fn_of(case), thr, False)
    return np.array([[tp[c], true[c], pred[c]] for c in range(case.class_num)], np.int64)


def reference_recall_precision(case):
    from yolov3_tensorflow_amd.utils import eval_utils
    return eval_utils._evaluate(y_pred_of(case), case.y_true, case.class_num, nms_fn_of(case), case.iou_thresh, True)


def _iou_of_first_pair(y_true, box):
    """calc_iou of one float32 detection with the first object of image 0, as _evaluate computes it."""
    from yolov3_tensorflow_amd.utils import eval_utils
    _, gt = eval_utils._ground_truth_of_image(y_true, 0)
    return float(eval_utils.calc_iou(np.asarray([box], np.float32), gt)[0, 0]), gt[0]


def _iou_all_float64(box, gt):
    p = np.asarray(box, np.float32).astype(np.float64)
    wh = np.maximum(np.minimum(p[2:], gt[2:]) - np.maximum(p[:2], gt[:2]), 0.)
    inter = wh[0] * wh[1]
    return float(inter / ((p[2] - p[0]) * (p[3] - p[1]) + (gt[2] - gt[0]) * (gt[3] - gt[1]) - inter + 1e-10))


def corner_cases(h, w, C):
    L0, L1, L2 = 0, 1 % C, C - 1
    two = C > 1
    out = {}

    def add(name, y_true, dets, iou_thresh=0.5, gt_cap=None, dropped=0, expect=None):
        boxes, labels, counts = pack(dets)
        out[name] = Case(name, C, h, w, y_true, boxes, labels, counts, float(iou_thresh), gt_cap, dropped, expect if two else None)

    # the best-IoU object has another label; a lower-IoU object of the detection's own label would pass the threshold
    y = empty_y_true(1, h, w, C)
    put(y, 0, 0, 1, 1, 0, (60, 60, 40, 40), {L0: 1.})
    put(y, 0, 1, 2, 3, 1, (64, 60, 40, 40), {L1: 1.})
    det = corners((60, 60, 40, 40))
    if two:
        from yolov3_tensorflow_amd.utils import eval_utils
        iou = eval_utils.calc_iou(np.asarray([det], np.float32), eval_utils._ground_truth_of_image(y, 0)[1])[0]
        assert iou[0] > iou[1] > 0.5
    add('argmax_before_label', y, [[(det, L1)]], expect=(0, 2, 1))

    # identical boxes, different labels: the first in gather order takes every detection
    y = empty_y_true(2, h, w, C)
    box = (50, 44, 30, 36)
    put(y, 0, 0, 0, 1, 2, box, {L1: 1.})
    put(y, 0, 2, 3, 2, 0, box, {L0: 1.})
    put(y, 1, 0, 0, 1, 2, box, {L0: 1.})
    put(y, 1, 2, 3, 2, 0, box, {L1: 1.})
    add('tie_across_scales', y, [[(corners(box), L0)], [(corners(box), L0)]], expect=(1, 4, 2))
    y = empty_y_true(3, h, w, C)
    put(y, 0, 1, 1, 2, 0, box, {L1: 1.})          # (row 1, column 2) comes before (row 2, column 0)
    put(y, 0, 1, 2, 0, 0, box, {L0: 1.})
    put(y, 1, 1, 3, 3, 0, box, {L0: 1.})          # one cell, anchors 0 and 2
    put(y, 1, 1, 3, 3, 2, box, {L1: 1.})
    put(y, 2, 2, 2, 1, 1, box, {L1: 1.})          # one row, columns 1 and 3
    put(y, 2, 2, 2, 3, 0, box, {L0: 1.})
    add('tie_inside_a_scale', y, [[(corners(box), L0)], [(corners(box), L0), (corners(box), L1)], [(corners(box), L0)]],
        expect=(1, 6, 4))

    # several detections on one object
    y = empty_y_true(1, h, w, C)
    box = (80, 64, 50, 40)
    put(y, 0, 1, 4, 5, 1, box, {L2: 1.})
    dets = [(corners(box, j), L2) for j in ((1, -1, 2, 0), (-2, 2, 0, 1), (0, 0, 0, 0), (3, 3, 3, 3))] + [(corners(box), L0)]
    add('one_hit_per_object', y, [dets], expect=(1, 1, 5) if L2 != L0 else None)

    # an IoU exactly at the threshold is no hit; just above the next float64 below it, it is
    y = empty_y_true(1, h, w, C)
    put(y, 0, 2, 5, 7, 2, (70.3, 55.7, 41.9, 33.3), {L1: 1.})
    det = [50.1, 40.2, 88.7, 70.9]
    thr, _ = _iou_of_first_pair(y, det)
    assert 0.3 < thr < 0.9
    add('strict_at_threshold', y, [[(det, L1)]], iou_thresh=thr, expect=(0, 1, 1))
    add('strict_below_threshold', y, [[(det, L1)]], iou_thresh=np.nextafter(thr, 0.), expect=(1, 1, 1))

    # the detection's width, height and area are float32 values that differ from the float64 ones
    y = empty_y_true(1, h, w, C)
    put(y, 0, 0, 2, 2, 1, (505.1, 449.3, 990.3, 880.9), {L0: 1.})
    det = [3.3, 2.7, 1000.7, 900.9]
    thr, gt = _iou_of_first_pair(y, det)
    p32 = np.asarray(det, np.float32)
    p64 = p32.astype(np.float64)
    assert float(p32[2] - p32[0]) != p64[2] - p64[0] and float(p32[3] - p32[1]) != p64[3] - p64[1]
    assert float((p32[2] - p32[0]) * (p32[3] - p32[1])) != (p64[2] - p64[0]) * (p64[3] - p64[1])
    assert _iou_all_float64(det, gt) != thr and 0.5 < thr < 1.      # an all-float64 kernel misses one of the next two
    add('f32_area_at_threshold', y, [[(det, L0)]], iou_thresh=thr, expect=(0, 1, 1))
    add('f32_area_below_threshold', y, [[(det, L0)]], iou_thresh=np.nextafter(thr, 0.), expect=(1, 1, 1))

    # a NaN box takes the argmax and is no hit; so does a box with one NaN coordinate
    y = empty_y_true(2, h, w, C)
    box = (40, 90, 30, 30)
    put(y, 0, 1, 0, 0, 0, box, {L2: 1.})
    put(y, 1, 0, 3, 3, 2, (90, 30, 40, 40), {L0: 1.})
    put(y, 1, 2, 0, 0, 0, box, {L2: 1.})
    nan = float('nan')
    add('nan_box', y, [[([nan] * 4, L2)], [([nan] * 4, L2), ([nan] + corners(box)[1:], L2), ([nan] * 4, L0)]], expect=(0, 3, 4))

    # images without objects, without detections, with neither; and the same alone in a batch
    y = empty_y_true(3, h, w, C)
    put(y, 1, 2, 15, 15, 2, box, {L1: 1.})
    put(y, 1, 0, 0, 0, 0, (100, 100, 20, 20), {L2: 1.})
    add('empty_images', y, [[(corners(box), L1), (corners(box, (1, 1, 1, 1)), L2)], [], []], expect=(0, 2, 2))
    y = empty_y_true(1, h, w, C)
    add('only_detections', y, [[(corners(box), L1), (corners(box), L1), (corners(box), L0)]], expect=(0, 0, 3))
    y = empty_y_true(1, h, w, C)
    put(y, 0, 1, 7, 7, 1, box, {L1: 1.})
    add('only_objects', y, [[]], expect=(0, 1, 0))

    # mix-up cells: two class entries, a last channel != 1 (larger than every class entry in one of them)
    y = empty_y_true(1, h, w, C)
    boxes = [(30, 30, 24, 24), (90, 30, 24, 30), (30, 90, 30, 24), (90, 90, 28, 28)]
    put(y, 0, 0, 0, 0, 1, boxes[0], {L1: 0.6, L0: 0.4}, mix=0.6)
    put(y, 0, 1, 5, 1, 0, boxes[1], {L0: 0.5, L2: 0.5}, mix=0.4)            # equal entries: the first one
    put(y, 0, 2, 9, 9, 2, boxes[2], {L2: 0.45, L1: 0.44}, mix=0.9)
    put(y, 0, 2, 9, 10, 0, boxes[3], {L2: 1.}, mix=1.)
    dets = [(corners(boxes[0], (1, 0, 0, 1)), L1), (corners(boxes[0]), L0), (corners(boxes[1]), L0), (corners(boxes[1]), L2),
            (corners(boxes[2], (0, 1, 1, 0)), L2), (corners(boxes[2]), L1), (corners(boxes[3]), L2)]
    add('mix_up_cells', y, [dets], expect=(4, 4, 7) if C > 2 else None)

    # more objects than a wavefront is wide, spread over every scale and both passes of the gather
    rng = np.random.RandomState(70)
    y = empty_y_true(2, h, w, C)
    slots = [(s, r, c, a) for s, (gh, gw) in enumerate(grids(h, w)) for r in range(gh) for c in range(gw) for a in range(3)]
    dets = [[], []]
    chosen = rng.permutation(len(slots))
    for k in range(70):
        s, r, c, a = slots[chosen[k]]
        box, label = (20. * (k % 10) + 8., 20. * (k // 10) + 8., 14., 13.), int(rng.randint(0, C))
        put(y, 0, s, r, c, a, box, {label: 1.})
        if k % 4:
            dets[0].append((corners(box, rng.uniform(-1.5, 1.5, 4)), label if k % 7 else (label + 1) % C))
        if k % 9 == 0:
            dets[0].append((corners(box, rng.uniform(-1., 1., 4)), label))
    for k in range(10):
        s, r, c, a = slots[chosen[100 + k]]
        put(y, 1, s, r, c, a, (30. * k + 10., 40., 20., 50.), {k % C: 1.})
        dets[1].append((corners((30. * k + 10., 40., 20., 50.), rng.uniform(-2., 2., 4)), k % C))
    assert max(chosen[:70]) >= 1024 > min(chosen[:70])
    add('seventy_objects', y, dets)
    add('gt_cap_overflow', y, dets, gt_cap=8, dropped=(70 - 8) + (10 - 8))
    return out


def random_case(h, w, C, n, seed):
    """n images with 0 .. 12 objects each in random cells; detections are jittered copies (some with another label, some
    twice) plus clutter.  Image 1 (when there is one) has no object, image 2 no detection."""
    rng = np.random.RandomState(1000 * seed + n)
    y = empty_y_true(n, h, w, C)
    slots = [(s, r, c, a) for s, (gh, gw) in enumerate(grids(h, w)) for r in range(gh) for c in range(gw) for a in range(3)]
    dets = []
    for i in range(n):
        k_i = 0 if i == 1 else int(rng.randint(1, 13))
        d = []
        for k, at in enumerate(rng.permutation(len(slots))[:k_i]):
            s, r, c, a = slots[at]
            wh = rng.uniform(16, 70, 2)
            box = (rng.uniform(wh[0] / 2, w - wh[0] / 2), rng.uniform(wh[1] / 2, h - wh[1] / 2), wh[0], wh[1])
            label = int(rng.randint(0, C))
            put(y, i, s, r, c, a, box, {label: 1.} if k % 3 else {label: 0.7, (label + 1) % C: 0.3}, mix=1. if k % 3 else 0.7)
            for _ in range(int(rng.randint(0, 3))):
                sigma = 2. if rng.uniform() < 0.6 else 9.
                d.append((corners(box, rng.normal(0, sigma, 4)), label if rng.uniform() < 0.8 else int(rng.randint(0, C))))
        for _ in range(int(rng.randint(0, 6))):
            x0, y0 = rng.uniform(0, w - 20), rng.uniform(0, h - 20)
            d.append(([x0, y0, x0 + rng.uniform(10, 60), y0 + rng.uniform(10, 60)], int(rng.randint(0, C))))
        dets.append([] if i == 2 else [d[k] for k in rng.permutation(len(d))])
    boxes, labels, counts = pack(dets)
    return Case('random_n%d_seed%d' % (n, seed), C, h, w, y, boxes, labels, counts, 0.5, None, 0, None)


_CACHE = {}


def all_cases(h, w, C):
    """name -> Case: every corner case and two random batches (n = 1 and n = 5), built once per (h, w, C)."""
    key = (h, w, C)
    if key not in _CACHE:
        cases = corner_cases(h, w, C)
        for n in (1, 5):
            case = random_case(h, w, C, n, seed=3)
            cases[case.name] = case
        _CACHE[key] = cases
    return _CACHE[key]


_REFERENCE = {}


def reference_of(case):
    """The expected table of a case, computed once (int64 [C, 3], read-only)."""
    key = (case.name, case.h, case.w, case.class_num)
    if key not in _REFERENCE:
        table = reference_table(case)
        table.setflags(write=False)
        _REFERENCE[key] = table
    return _REFERENCE[key]
