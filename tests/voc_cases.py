"""Shared inputs and checks of tests/test_voc_device_cpu.py (the evaluator's arithmetic on the host) and
tests/test_voc_device_gpu.py (the kernels): the committed reference vectors, seeded random sets, the corner cases, and the
comparison with eval_utils.voc_eval.  A case is (gt_dict, image_ids, preds, class_num) with preds the rows
[image_id, x_min, y_min, x_max, y_max, score, label] of get_preds_gpu, in arrival order."""
import collections
import contextlib
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

Case = collections.namedtuple('Case', 'gt_dict image_ids preds class_num')


def golden():
    g = np.load(os.path.join(HERE, 'golden', 'reference_eval_goldens.npz'))
    gd = {}
    for row in g['gt_rec_lb1']:
        gd.setdefault(int(row[0]), []).append([row[1], row[2], row[3], row[4], int(row[5])])
    preds = [[int(r[0]), r[1], r[2], r[3], r[4], r[5], int(r[6])] for r in g['voc_preds']]
    return Case(gd, sorted(gd), preds, 6), g['voc_results']


def random_case(seed, images=40, classes=5, fp32=True):
    """About 600 detections: jittered ground truth, duplicates and clutter; 0-12 objects per image; scores distinct.
    fp32: boxes and scores are fp32 numbers (what the NMS kernels emit), so the same set runs through y3_voc_append."""
    rng = np.random.RandomState(seed)
    gd, preds = {}, []
    for img in range(images):
        objs = []
        for _ in range(int(rng.randint(0, 13))):
            x0, y0 = rng.uniform(0, 300, 2)
            objs.append([x0, y0, x0 + rng.uniform(8, 110), y0 + rng.uniform(8, 110), int(rng.randint(0, classes))])
        gd[100 + 3 * img] = objs
        for o in objs:
            for _ in range(int(rng.randint(0, 3))):
                j = rng.normal(0, 5.0, 4)
                preds.append([100 + 3 * img, o[0] + j[0], o[1] + j[1], o[2] + j[2], o[3] + j[3], 0., o[4]])
        for _ in range(int(rng.randint(3, 12))):
            x0, y0 = rng.uniform(0, 300, 2)
            preds.append([100 + 3 * img, x0, y0, x0 + rng.uniform(8, 110), y0 + rng.uniform(8, 110), 0., int(rng.randint(0, classes))])
    scores = rng.permutation(np.linspace(0.02, 0.98, len(preds)))
    for p, s in zip(preds, scores):
        p[5] = s
    if fp32:
        preds = [[p[0]] + [float(np.float32(v)) for v in p[1:6]] + [p[6]] for p in preds]
    return Case(gd, sorted(gd), preds, classes)


def assert_distinct_scores(case):
    for c in range(case.class_num):
        s = [p[5] for p in case.preds if p[6] == c]
        assert len(set(s)) == len(s), 'class %d has tied scores' % c


def corner_cases():
    """name -> (Case, expectation or None).  Expectations are (class, tp flags in rank order)."""
    out = {}
    # IoU exactly 0.5 is a false positive: [0,0,9,9] against [0,0,9,19] is 100 / 200 with the +1 convention
    out['iou_exactly_half'] = Case({1: [[0., 0., 9., 19., 0]]}, [1], [[1, 0., 0., 9., 9., .9, 0]], 1), (0, [0])
    # two detections whose best object is A; B also passes the threshold for the second one and stays unclaimed: no second choice
    a, b = [0., 0., 99., 99., 0], [0., 10., 99., 109., 0]
    out['no_second_choice'] = Case({1: [a, b]}, [1], [[1, 0., 0., 99., 99., .9, 0], [1, 0., 2., 99., 101., .8, 0]], 1), (0, [1, 0])
    # duplicate object boxes: the first index is the arg-max, so the second detection finds it claimed
    out['duplicate_objects'] = Case({1: [list(a), list(a)]}, [1], [[1, 0., 0., 99., 99., .9, 0], [1, 0., 0., 99., 99., .8, 0]], 1), (0, [1, 0])
    # an image without objects of the class, an image without any object
    out['empty_images'] = Case({1: [[0., 0., 50., 50., 1]], 2: [], 3: [[0., 0., 50., 50., 0]]}, [1, 2, 3],
                               [[1, 0., 0., 50., 50., .9, 0], [2, 0., 0., 50., 50., .8, 0], [3, 0., 0., 50., 50., .7, 0],
                                [1, 1., 1., 50., 50., .6, 1]], 2), (0, [0, 0, 1])
    # detections of a class that has no object anywhere: recall and the area AP are NaN, precision 0
    out['npos_zero'] = Case({1: [[0., 0., 50., 50., 0]]}, [1], [[1, 0., 0., 50., 50., .9, 1], [1, 5., 5., 40., 40., .8, 1],
                                                                 [1, 0., 0., 50., 50., .7, 0]], 3), (1, [0, 0])
    return out


def tied_case(seed=11):
    """The random set with scores quantised to a handful of values, so that most ranks inside a class are decided by row."""
    c = random_case(seed, images=12, classes=3)
    preds = [[p[0]] + p[1:5] + [float(np.float32(round(p[5] * 6) / 6.))] + [p[6]] for p in c.preds]
    return Case(c.gt_dict, c.image_ids, preds, c.class_num)


def voc_eval_stable(gt_dict, val_preds, classidx, iou_thres=0.5, use_07_metric=False):
    """eval_utils.voc_eval restated with the one change the device order makes: a stable descending sort (ties keep arrival
    order).  For distinct scores it is voc_eval."""
    from yolov3_tensorflow_amd.utils.eval_utils import voc_ap
    gt = {k: np.array([o[:4] for o in v if o[-1] == classidx], np.float64).reshape(-1, 4) for k, v in gt_dict.items()}
    used = {k: np.zeros(len(v), bool) for k, v in gt.items()}
    npos = sum(len(v) for v in gt.values())
    pred = [p for p in val_preds if p[-1] == classidx]
    if not pred:
        return 1e-6, 1e-6, 0, 0, 0
    order = np.argsort(-np.array([p[-2] for p in pred]), kind='stable')
    nd = len(pred)
    tp = np.zeros(nd)
    for rank, k in enumerate(order):
        g, bb = gt[pred[k][0]], np.array(pred[k][1:5], np.float64)
        if g.size == 0:
            continue
        iw = np.maximum(np.minimum(g[:, 2], bb[2]) - np.maximum(g[:, 0], bb[0]) + 1., 0.)
        ih = np.maximum(np.minimum(g[:, 3], bb[3]) - np.maximum(g[:, 1], bb[1]) + 1., 0.)
        inters = iw * ih
        uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.) - inters)
        overlaps = inters / uni
        j = int(np.argmax(overlaps))
        if overlaps[j] > iou_thres and not used[pred[k][0]][j]:
            used[pred[k][0]][j] = True
            tp[rank] = 1.
    fp = np.cumsum(1. - tp)
    tp = np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return npos, nd, tp[-1] / float(npos), tp[-1] / float(nd), voc_ap(rec, prec, use_07_metric)


def reference_table(case, iou_thres, use_07_metric, fn=None):
    from yolov3_tensorflow_amd.utils import eval_utils
    fn = fn or eval_utils.voc_eval
    rows = []
    with np.errstate(all='ignore'), contextlib.redirect_stdout(io.StringIO()):
        for c in range(case.class_num):
            rows.append([float(v) for v in fn(case.gt_dict, case.preds, c, iou_thres=iou_thres, use_07_metric=use_07_metric)])
    return np.array(rows, np.float64)


def assert_table(got, want, use_07_metric, what=''):
    """npos, nd, recall, precision and the 11-point AP bit for bit (NaN equal to NaN); the area AP within nd * 2**-52, the bound
    on two summation orders of non-negative float64 terms whose sum is at most 1."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    for c, (g, w) in enumerate(zip(got, want)):
        print(what, 'class', c, 'got', g.tolist(), 'want', w.tolist())
        np.testing.assert_array_equal(g[:4], w[:4], err_msg='%s class %d' % (what, c))      # (treats NaN as equal to NaN)
        if use_07_metric or np.isnan(w[4]):
            np.testing.assert_array_equal(g[4], w[4], err_msg='%s class %d AP' % (what, c))
        else:
            assert abs(g[4] - w[4]) <= w[1] * 2.0 ** -52, '%s class %d area AP %r vs %r' % (what, c, g[4], w[4])


def arena_of(case):
    """The arena rows and the ground-truth CSR of a case as numpy arrays (image index = position in image_ids)."""
    index = {k: i for i, k in enumerate(case.image_ids)}
    p = case.preds
    box = np.array([r[1:5] for r in p], np.float64).reshape(-1, 4)
    score = np.array([r[5] for r in p], np.float64)
    label = np.array([r[6] for r in p], np.int32)
    image = np.array([index[r[0]] for r in p], np.int32)
    starts, gbox, glab = [0], [], []
    for k in case.image_ids:
        for o in case.gt_dict[k]:
            gbox.append(o[:4])
            glab.append(o[4])
        starts.append(len(glab))
    return dict(box=box, score=score, label=label, image=image, gt_start=np.array(starts, np.int32),
                gt_box=np.array(gbox or [[0.] * 4], np.float64).reshape(-1, 4), gt_label=np.array(glab or [-1], np.int32),
                num_gt=len(glab), num_images=len(case.image_ids))
