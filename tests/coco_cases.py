"""Shared inputs and checks of tests/test_coco_device_cpu.py (the COCO evaluator's arithmetic on the host) and
tests/test_coco_device_gpu.py (the kernels): the five hand-worked pins, seeded random sets, the corner cases, and the comparison
with eval_utils.coco_eval.  A case is (gt_dict, image_ids, preds, class_num, area_scale) with gt_dict in image_ids order (its
order is coco_eval's image order), preds the rows [image_id, x_min, y_min, x_max, y_max, score, label] of get_preds_batch in
arrival order, and area_scale None or {image_id: factor}."""
import collections
import functools

import numpy as np

Case = collections.namedtuple('Case', 'gt_dict image_ids preds class_num area_scale')
EPS = 2.220446049250313e-16
ONE = 1. / (1. + EPS)          # the precision of a lone true positive: 0.9999999999999998


def case(gts, dets, class_num=1, area_scale=None):
    """gts: {image_id: [[x0, y0, x1, y1, label], ...]} (insertion order = image order); dets: rows as above."""
    gd = {k: [list(map(float, o[:4])) + [int(o[4])] for o in v] for k, v in gts.items()}
    return Case(gd, list(gd), [[d[0]] + [float(v) for v in d[1:6]] + [int(d[6])] for d in dets], class_num, area_scale)


def pins():
    """name -> (Case, the twelve expected numbers): hand-worked from the rule (include/yolo355.h), one class."""
    c_ap = 51 * 0.5 / 101
    out = {}
    out['A'] = (case({1: [[0, 0, 10, 10, 0]]}, [[1, 0, 0, 10, 10, .9, 0]]),
                [ONE, ONE, ONE, ONE, -1, -1, 1, 1, 1, 1, -1, -1])
    # IoU exactly 0.5: a match at the first threshold only
    out['B'] = (case({1: [[0, 0, 2, 1, 0]]}, [[1, 0, 0, 1, 1, .9, 0]]),
                [ONE / 10, ONE, 0, ONE / 10, -1, -1, .1, .1, .1, .1, -1, -1])
    # a false positive in front of the one true positive of two objects: 1 / (2 + eps) is 0.5 exactly, reached by 51 thresholds
    out['C'] = (case({1: [[0, 0, 10, 10, 0], [50, 50, 60, 60, 0]]},
                     [[1, 100, 100, 110, 110, .9, 0], [1, 0, 0, 10, 10, .8, 0]]),
                [c_ap, c_ap, c_ap, c_ap, -1, -1, 0, .5, .5, .5, -1, -1])
    # an area of exactly 32^2 is small and medium; the large unmatched detection is ignored there and a false positive in "all"
    out['D'] = (case({1: [[0, 0, 32, 32, 0]]}, [[1, 0, 0, 32, 32, .9, 0], [1, 200, 200, 400, 400, .8, 0]]),
                [ONE, ONE, ONE, ONE, ONE, -1, 1, 1, 1, 1, 1, -1])
    # two identical objects, three identical detections: 2 / (2 + eps) is 1.0, and the envelope carries it to the front
    out['E'] = (case({1: [[0, 0, 10, 10, 0], [0, 0, 10, 10, 0]]},
                     [[1, 0, 0, 10, 10, .9, 0], [1, 0, 0, 10, 10, .8, 0], [1, 0, 0, 10, 10, .7, 0]]),
                [1., 1., 1., 1., -1, -1, .5, 1, 1, 1, -1, -1])
    return out


def _f32(v):
    return float(np.float32(v))


def random_case(seed, images=12, classes=4, fp32=True, quantise=True):
    """A few hundred detections: jittered ground truth, duplicates and clutter over objects of all three sizes, 0-9 objects
    per image (some images empty); part of the scores quantised, so that ties inside a group and across images occur.
    fp32: boxes and scores are fp32 numbers (what the NMS kernels emit), so the same set runs through y3_voc_append."""
    rng = np.random.RandomState(seed)
    gts, dets = {}, []
    for img in range(images):
        objs = []
        for _ in range(int(rng.randint(0, 10)) if img % 5 != 4 else 0):
            x0, y0 = rng.uniform(0, 250, 2)
            side = float(rng.choice([rng.uniform(8, 30), rng.uniform(34, 90), rng.uniform(100, 160)]))
            objs.append([x0, y0, x0 + side, y0 + side * rng.uniform(0.7, 1.3), int(rng.randint(0, classes))])
        gts[50 + 7 * img] = objs
    ids = list(gts)
    for img in rng.permutation(ids):          # (arrival order is not the image order)
        for o in gts[img]:
            for _ in range(int(rng.randint(0, 4))):
                j = rng.normal(0, 0.06 * (o[2] - o[0]), 4)
                dets.append([img, o[0] + j[0], o[1] + j[1], o[2] + j[2], o[3] + j[3], 0., o[4]])
        for _ in range(int(rng.randint(2, 9))):
            x0, y0 = rng.uniform(0, 250, 2)
            side = rng.uniform(8, 160)
            dets.append([img, x0, y0, x0 + side, y0 + side, 0., int(rng.randint(0, classes))])
    scores = rng.permutation(np.linspace(0.02, 0.98, len(dets)))
    for d, s in zip(dets, scores):
        d[5] = round(s * 8) / 8. if quantise and rng.uniform() < 0.4 else s
    if fp32:
        dets = [[d[0]] + [_f32(v) for v in d[1:6]] + [d[6]] for d in dets]
    return case(gts, dets, classes)


@functools.lru_cache(maxsize=None)
def corner_cases():
    """name -> Case; what each is for is said next to it.  Built once."""
    out = {}
    for name, (c, _) in pins().items():
        out['pin_' + name] = c
    # IoU exactly 1/2 and exactly 3/4: linspace gives exactly 0.5 and 0.75 at indices 0 and 5, and an equal IoU matches
    out['iou_exactly_threshold'] = case({1: [[0, 0, 2, 1, 0]], 2: [[0, 0, 4, 1, 0]]},
                                        [[1, 0, 0, 1, 1, .9, 0], [2, 0, 0, 3, 1, .8, 0]])
    # equal IoUs (2/3) to two objects: the later one is taken, so the second detection still finds the first object
    out['equal_ious_later_wins'] = case({1: [[-2, 0, 8, 10, 0], [2, 0, 12, 10, 0]]},
                                        [[1, 0, 0, 10, 10, .9, 0], [1, -2, 0, 8, 10, .8, 0]])
    # "small": the object of IoU 0.75 counts and the better one (0.909) is ignored: the detection takes the first at t <= 0.75,
    # the ignored one above that; "all": it takes the better one
    out['non_ignored_before_better_ignored'] = case({1: [[0, 0, 30, 30, 0], [0, 0, 40, 33, 0]]}, [[1, 0, 0, 40, 30, .9, 0]])
    # areas of exactly 32^2 and 96^2 sit in two ranges each
    out['areas_on_the_boundaries'] = case({1: [[0, 0, 32, 32, 0], [200, 200, 296, 296, 0]]},
                                          [[1, 0, 0, 32, 32, .9, 0], [1, 200, 200, 296, 296, .8, 0], [1, 0, 100, 31, 133, .7, 0]])
    # area_scale 1.5 moves a 30 x 30 object (900: small) to 1350 (medium); image 2 keeps 1.0
    out['area_scale_moves_an_object'] = case({1: [[0, 0, 30, 30, 0]], 2: [[0, 0, 30, 30, 0]]},
                                             [[1, 1, 0, 30, 30, .9, 0], [2, 0, 1, 30, 30, .8, 0]], area_scale={1: 1.5, 2: 1.0})
    # classes: 0 objects and detections, 1 objects only (precision 0, recall 0), 2 detections only (-1), 3 neither; image 3 has
    # no object at all and still detections
    out['empty_classes_and_images'] = case({1: [[0, 0, 50, 50, 0], [60, 60, 90, 90, 1]], 3: [], 5: [[10, 10, 80, 80, 0]]},
                                           [[1, 0, 0, 50, 52, .9, 0], [3, 0, 0, 50, 50, .8, 0], [3, 5, 5, 40, 40, .7, 2],
                                            [5, 10, 10, 80, 84, .6, 0], [1, 0, 0, 20, 20, .5, 2]], class_num=4)
    # equal scores across images (the image order decides, not the arrival order) and inside a group (the arrival order decides)
    out['tied_scores'] = case({1: [[0, 0, 10, 10, 0]], 2: [[0, 0, 10, 10, 0]], 3: [[0, 0, 10, 10, 0], [20, 0, 30, 10, 0]]},
                              [[3, 20, 0, 30, 10, .5, 0], [3, 100, 0, 110, 10, .5, 0], [2, 50, 50, 60, 60, .5, 0],
                               [1, 0, 0, 10, 10, .5, 0], [3, 0, 0, 10, 11, .5, 0], [2, 0, 0, 10, 10, .5, 0]])
    # 260 detections in one group: only the first 100 are matched, the in-group rank saturates at 255, and the one good
    # detection of the third object is the last of them; a second class and image ride along
    rng = np.random.RandomState(3)
    objs = [[0, 0, 40, 40, 0], [100, 0, 140, 40, 0], [0, 100, 40, 140, 0]]
    dets = [[1, 0, 1, 40, 40, 0., 0], [1, 100, 0, 141, 40, 0., 0]]
    for _ in range(257):
        x0, y0 = rng.uniform(200, 400, 2)          # (clutter away from the objects)
        dets.append([1, x0, y0, x0 + rng.uniform(10, 60), y0 + rng.uniform(10, 60), 0., 0])
    dets.append([1, 0, 100, 40, 140, 0., 0])
    for d, s in zip(dets, np.linspace(0.99, 0.01, len(dets))):
        d[5] = _f32(s)
    dets = [[d[0]] + [_f32(v) for v in d[1:5]] + d[5:] for d in dets]
    dets += [[2, 0, 0, 30, 30, .5, 1], [2, 0, 0, 31, 30, .25, 0]]
    out['more_than_100_detections'] = case({1: objs, 2: [[0, 0, 30, 30, 1], [0, 0, 30, 30, 0]]}, rng.permutation(np.array(dets, object)).tolist(), 2)
    # 70 objects of one class in one image: past one wavefront's width of objects
    rng = np.random.RandomState(8)
    objs, dets = [], []
    for k in range(70):
        x0, y0 = 40. * (k % 10), 40. * (k // 10)
        objs.append([x0, y0, x0 + 30., y0 + 30. + (k % 3) * 4, 0])
    for k in rng.permutation(70)[:60]:
        o = objs[k]
        dets.append([7, o[0] + 1., o[1] - 1., o[2] + 2., o[3], 0., 0])
        if k % 3 == 0:
            dets.append([7, o[0] - 2., o[1] + 2., o[2], o[3] + 1., 0., 0])
    for _ in range(15):
        x0, y0 = rng.uniform(0, 400, 2)
        dets.append([7, x0, y0, x0 + 30., y0 + 30., 0., 0])
    for d, s in zip(dets, rng.permutation(np.linspace(0.05, 0.95, len(dets)))):
        d[5] = _f32(s)
    out['seventy_objects_in_one_group'] = case({7: objs, 9: []}, dets)
    return out


@functools.lru_cache(maxsize=None)
def many_objects_case(n_objects):
    """One image with n_objects objects of two classes (more than the kernel keeps "taken" words for in the LDS) and a few
    dozen detections; a second, ordinary image."""
    rng = np.random.RandomState(5)
    objs, dets = [], []
    for k in range(n_objects):
        x0, y0 = 25. * (k % 40), 25. * (k // 40)
        objs.append([x0, y0, x0 + 20., y0 + 20. + (k % 2) * 16, k % 2])
    for k in rng.permutation(n_objects)[:40]:
        o = objs[k]
        dets.append([1, o[0] + 1., o[1], o[2], o[3] + 1., 0., o[4]])
        if k % 4 == 0:
            dets.append([1, o[0], o[1] + 1., o[2] - 1., o[3], 0., o[4]])
    dets += [[2, 0., 0., 50., 50., 0., 0], [2, 5., 5., 50., 50., 0., 0]]
    for d, s in zip(dets, rng.permutation(np.linspace(0.05, 0.95, len(dets)))):
        d[5] = _f32(s)
    return case({1: objs, 2: [[0, 0, 50, 50, 0]]}, dets, 2)


@functools.lru_cache(maxsize=None)
def long_case(pass_len):
    """Class 0's list is two passes of the AP kernel plus a few ranks (25 images of at most 100 detections each); classes 1
    and 2 ride behind it."""
    rng = np.random.RandomState(21)
    images = (2 * pass_len + 40) // 90 + 1
    gts, dets = {}, []
    for img in range(images):
        objs = []
        for _ in range(6):
            x0, y0 = rng.uniform(0, 300, 2)
            objs.append([x0, y0, x0 + rng.uniform(15, 120), y0 + rng.uniform(15, 120), int(rng.randint(0, 3) == 2) * int(rng.randint(1, 3))])
        gts[img] = objs
        for _ in range(90):
            o = objs[int(rng.randint(0, 6))]
            j = rng.normal(0, 5.0, 4) if rng.uniform() < 0.4 else rng.uniform(-50, 50, 4)
            dets.append([img, o[0] + j[0], o[1] + j[1], o[2] + j[2], o[3] + j[3], 0., 0])
        for _ in range(4):
            o = objs[int(rng.randint(0, 6))]
            dets.append([img, o[0] + 1., o[1], o[2], o[3] + 2., 0., int(rng.randint(1, 3))])
    scores = np.unique(rng.uniform(0.01, 0.99, 2 * len(dets)).astype(np.float32))
    for d, s in zip(dets, rng.permutation(scores)[:len(dets)]):
        d[5] = float(s)
    dets = [[d[0]] + [_f32(v) for v in d[1:5]] + d[5:] for d in dets]
    c = case(gts, dets, 3)
    assert sum(d[6] == 0 for d in c.preds) > 2 * pass_len
    return c


def voc_comparable_case(seed=4, images=16, classes=3):
    """Every detection overlaps at most one object of its class (objects sit alone in 120-pixel cells, a detection stays in the
    cell of its object or in an empty one), and no IoU, with the +1 convention or without, lies in [0.45, 0.55]."""
    from yolov3_tensorflow_amd.utils.eval_utils import COCO_IOU_THRS      # noqa: F401 (the package is importable)
    rng = np.random.RandomState(seed)
    gts, dets = {}, []
    for img in range(images):
        objs, cells = [], rng.permutation(9)
        for cell in cells[:int(rng.randint(2, 7))]:
            x0, y0 = 120. * (cell % 3) + 30, 120. * (cell // 3) + 30
            o = [x0, y0, x0 + rng.uniform(30, 60), y0 + rng.uniform(30, 60), int(rng.randint(0, classes))]
            objs.append(o)
            for _ in range(int(rng.randint(0, 4))):
                j = rng.uniform(-14, 14, 4)
                dets.append([img, o[0] + j[0], o[1] + j[1], o[2] + j[2], o[3] + j[3], 0., o[4]])
        for cell in cells[7:]:
            x0, y0 = 120. * (cell % 3) + 30, 120. * (cell // 3) + 30
            dets.append([img, x0, y0, x0 + 40, y0 + 40, 0., int(rng.randint(0, classes))])
        gts[img] = objs

    def ious(d, o):
        out = []
        for one in (0., 1.):
            w = min(d[3], o[2]) - max(d[1], o[0]) + one
            h = min(d[4], o[3]) - max(d[2], o[1]) + one
            inter = max(w, 0.) * max(h, 0.)
            out.append(inter / ((d[3] - d[1] + one) * (d[4] - d[2] + one) + (o[2] - o[0] + one) * (o[3] - o[1] + one) - inter))
        return out
    dets = [d for d in dets if all(not 0.45 <= v <= 0.55 for o in gts[d[0]] for v in ious(d, o))]
    for d, s in zip(dets, rng.permutation(np.linspace(0.05, 0.95, len(dets)))):
        d[5] = s
    return case(gts, dets, classes), ious


def reference(c):
    from yolov3_tensorflow_amd.utils.eval_utils import coco_eval
    return coco_eval(c.gt_dict, c.preds, c.class_num, c.area_scale)


def entries_averaged(want):
    """How many entries each of the twelve numbers averages: (stats [12], per_class [K, 12])."""
    p, r = want['precision'], want['recall']

    def counts(p, r):
        slices = [p[:, :, :, 0, 2], p[0, :, :, 0, 2], p[5, :, :, 0, 2]] + [p[:, :, :, a, 2] for a in (1, 2, 3)]
        slices += [r[:, :, 0, m] for m in (0, 1, 2)] + [r[:, :, a, 2] for a in (1, 2, 3)]
        return np.array([int((s > -1).sum()) for s in slices])
    K = p.shape[2]
    return counts(p, r), np.stack([counts(p[:, :, k:k + 1], r[:, k:k + 1]) for k in range(K)])


def assert_result(got, want, what=''):
    """precision and recall bit for bit; the twelve numbers, overall and per class, within n * 2**-52 of the oracle's mean over
    the n entries they average: the bound on two summation orders of n non-negative float64 terms of at most 1, divided by n
    (-1, "nothing defined", exactly)."""
    if 'precision' in got:
        np.testing.assert_array_equal(got['precision'], want['precision'], err_msg=what + ' precision')
        np.testing.assert_array_equal(got['recall'], want['recall'], err_msg=what + ' recall')
    n_stats, n_class = entries_averaged(want)
    for name, g, w, n in (('stats', got['stats'], want['stats'], n_stats), ('per_class', got['per_class'], want['per_class'], n_class)):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape, what
        print(what, name, 'largest gap', float(np.abs(g - w).max()), 'entries', n.max())
        np.testing.assert_array_equal(g[w == -1], w[w == -1], err_msg='%s %s undefined entries' % (what, name))
        assert (np.abs(g - w) <= n * 2.0 ** -52).all(), '%s %s: %r vs %r' % (what, name, g, w)


def arena_of(c):
    """The arena rows and the ground-truth CSR of a case as numpy arrays (image index = position in image_ids)."""
    index = {k: i for i, k in enumerate(c.image_ids)}
    p = c.preds
    starts, gbox, glab = [0], [], []
    for k in c.image_ids:
        for o in c.gt_dict[k]:
            gbox.append(o[:4])
            glab.append(o[4])
        starts.append(len(glab))
    scale = None if c.area_scale is None else np.array([float(c.area_scale[k]) for k in c.image_ids], np.float64)
    return dict(box=np.array([r[1:5] for r in p], np.float64).reshape(-1, 4), score=np.array([r[5] for r in p], np.float64),
                label=np.array([r[6] for r in p], np.int32), image=np.array([index[r[0]] for r in p], np.int32),
                gt_start=np.array(starts, np.int32), gt_box=np.array(gbox or [[0.] * 4], np.float64).reshape(-1, 4),
                gt_label=np.array(glab or [-1], np.int32), num_gt=len(glab), num_images=len(c.image_ids), area_scale=scale)
