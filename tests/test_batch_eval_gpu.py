"""GPU tests of the training-batch evaluator: y3_batch_eval (include/yolo355.h) with hand-loaded detection tensors over every
case of tests/beval_cases.py, and eval_utils.evaluate_on_device against evaluate_on_gpu.  The expected value is
eval_utils._evaluate everywhere; the three per-class count vectors are compared for exact equality and calc_now=True's two
floats bit for bit.  Plus what only the kernels have: the real cell count (several passes of the gather), accumulation into
one table, run-to-run identity, and poison in the dead slots and in the scratch."""
import functools

import numpy as np
import pytest

import beval_cases as bc

pytestmark = pytest.mark.gpu

SIZES = [(160, 128), (128, 160)]
CLASSES = [1, 3, 80]


def _upload(case):
    import torch
    from yolov3_tensorflow_amd import framework as fw
    dev = fw.default_device()
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (case.boxes, case.labels, case.counts) + tuple(case.y_true))


def _entry(case, on_dev=None, table=None, scratch_fill=0xA5, slack=64):
    """One y3_batch_eval call: (table int64 [C, 3] on the host, the overflow word).  The scratch is filled with
    `scratch_fill` and followed by `slack` guard bytes that must come back untouched."""
    import torch
    from yolov3_tensorflow_amd import _lib, framework as fw
    L, dev = _lib.lib(), fw.default_device()
    ob, ol, cnt, y1, y2, y3 = on_dev if on_dev is not None else _upload(case)
    n, cap, C = int(ob.shape[0]), int(ob.shape[1]), case.class_num
    gt_cap = case.gt_cap if case.gt_cap is not None else min(bc.cells_of_image(case.h, case.w), 4096)
    nbytes = L.y3_batch_eval_scratch_bytes(n, gt_cap)
    assert nbytes > 0
    scratch = torch.full((nbytes + slack,), scratch_fill, dtype=torch.uint8, device=dev)
    if table is None:
        table = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    state = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.y3_batch_eval(fw.context(dev), fw.ptr(ob), fw.ptr(ol), fw.ptr(cnt), n, cap, fw.ptr(y1), fw.ptr(y2), fw.ptr(y3),
                               case.h, case.w, C, case.iou_thresh, gt_cap, fw.ptr(scratch), nbytes, fw.ptr(table), fw.ptr(state)))
    host = table.cpu().numpy()
    fw.check_context(dev)
    assert (scratch[nbytes:] == scratch_fill).all()
    return host, int(state.item())


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_every_case_through_the_entry(size, C):
    cases = bc.all_cases(size[0], size[1], C)
    assert {len(c.counts) for c in cases.values()} >= {1, 5}
    for name, case in sorted(cases.items()):
        got, dropped = _entry(case)
        assert dropped == case.dropped, name
        if case.dropped:
            continue
        np.testing.assert_array_equal(got, bc.reference_of(case), err_msg=name)


def test_the_real_cell_count():
    """416x416, 80 classes, n = 2: 10,647 cells per image are eleven passes of the gather; 70 objects spread over them."""
    case = bc.corner_cases(416, 416, 80)['seventy_objects']
    assert bc.cells_of_image(416, 416) == 10647 and len(case.counts) == 2
    got, dropped = _entry(case)
    want = bc.reference_table(case)
    assert dropped == 0 and want[:, 1].sum() == 80 and want[:, 0].sum() > 20
    np.testing.assert_array_equal(got, want)


def test_accumulation_identity_and_poison():
    import torch
    a, b = bc.all_cases(160, 128, 3)['random_n5_seed3'], bc.all_cases(160, 128, 3)['seventy_objects']
    ta, tb = _entry(a)[0], _entry(b)[0]
    np.testing.assert_array_equal(ta, bc.reference_of(a))
    # two batches into one table = the sum of two tables
    on_dev = _upload(a)
    table = torch.zeros((3, 3), dtype=torch.int64, device=on_dev[0].device)
    _entry(a, on_dev, table=table)
    both, _ = _entry(b, table=table)
    np.testing.assert_array_equal(both, ta + tb)
    # the same call three times: identical tables
    for _ in range(3):
        np.testing.assert_array_equal(_entry(b)[0], tb)
    # other poison in the scratch and in the slots past each count
    for fill in (0x00, 0xFF, 0x7F):
        np.testing.assert_array_equal(_entry(b, scratch_fill=fill)[0], tb)
    boxes, labels = b.boxes.copy(), b.labels.copy()
    for i, k in enumerate(b.counts):
        boxes[i, k:], labels[i, k:] = boxes[i, 0], labels[i, 0]
    np.testing.assert_array_equal(_entry(b._replace(boxes=boxes, labels=labels))[0], tb)
    labels[0, b.counts[0]:] = 1 << 30
    boxes[1, b.counts[1]:] = np.inf
    np.testing.assert_array_equal(_entry(b._replace(boxes=boxes, labels=labels))[0], tb)


def _seeded_y_pred(case, boxes_per_image, seed):
    """y_pred of a batch whose y_true is the case's: noisy copies of the objects (twice), a wrong-class copy, clutter; conf
    and probs distinct (what tests/golden/make_golden.py builds for evaluate_on_cpu)."""
    from yolov3_tensorflow_amd.utils import eval_utils
    rng = np.random.RandomState(seed)
    n, C, M = len(case.counts), case.class_num, boxes_per_image
    pb, pc, pp = np.empty((n, M, 4), np.float32), np.empty((n, M, 1), np.float32), np.empty((n, M, C), np.float32)
    for i in range(n):
        labels, gt = eval_utils._ground_truth_of_image(case.y_true, i)
        K = len(labels)
        assert 2 * K < M
        xy = rng.uniform(0, 100, (M, 2))
        pb[i] = np.concatenate([xy, xy + rng.uniform(8, 60, (M, 2))], 1)
        pb[i, :K] = gt + rng.normal(0, 3.0, (K, 4))
        pb[i, K:2 * K] = gt + rng.normal(0, 1.5, (K, 4))
        conf = ((rng.permutation(M) + 0.5) / M).astype(np.float32).reshape(M, 1)
        conf[:2 * K] = 0.5 + conf[:2 * K] / 2
        probs = (((rng.permutation(M * C) + 0.5) / (M * C)) * 0.3).astype(np.float32).reshape(M, C)
        lab = np.concatenate([labels, labels, rng.randint(0, C, M - 2 * K)]).astype(np.int64)
        if K:
            lab[K] = (lab[K] + 1) % C
        probs[np.arange(M), lab] += np.float32(0.7)
        pc[i], pp[i] = conf, probs
    return pb, pc, pp


@pytest.mark.parametrize('config', [(5, 6, 20, 0.3, 0.45), (2, 80, 150, 0.01, 0.45)], ids=['nms_20_0.3', 'train_defaults'])
def test_evaluate_on_device_equals_evaluate_on_gpu(config):
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils import eval_utils
    from yolov3_tensorflow_amd.utils.nms_utils import gpu_nms
    n, C, max_boxes, score_thresh, nms_thresh = config
    case = bc.random_case(160, 128, C, n, seed=11)
    y_pred = tuple(torch.from_numpy(a).to(fw.default_device()) for a in _seeded_y_pred(case, 60, seed=n))
    y_true = [torch.from_numpy(t).to(fw.default_device()) for t in case.y_true]
    op = functools.partial(gpu_nms, num_classes=C, max_boxes=max_boxes, score_thresh=score_thresh, nms_thresh=nms_thresh)
    with_scores = (y_pred[0], y_pred[1] * y_pred[2])
    for iou_thresh in (0.5, nms_thresh):
        want = eval_utils.evaluate_on_gpu(None, op, None, None, y_pred, y_true, C, iou_thresh, calc_now=False)
        assert sum(want[0].values()) > 0 and sum(want[2].values()) > sum(want[0].values())      # hits and false positives
        rec, prec = eval_utils.evaluate_on_gpu(None, op, None, None, y_pred, y_true, C, iou_thresh, calc_now=True)
        for form in (y_pred, with_scores, tuple(a.cpu().numpy() for a in y_pred)):
            kw = dict(max_boxes=max_boxes, score_thresh=score_thresh, nms_thresh=nms_thresh, iou_thresh=iou_thresh)
            assert eval_utils.evaluate_on_device(form, y_true, C, calc_now=False, **kw) == want
            got = eval_utils.evaluate_on_device(form, y_true, C, **kw)
            assert np.float64(got[0]).tobytes() == np.float64(rec).tobytes()
            assert np.float64(got[1]).tobytes() == np.float64(prec).tobytes()


def test_evaluate_on_device_raises_when_gt_cap_is_too_small():
    from yolov3_tensorflow_amd.utils import eval_utils
    case = bc.all_cases(160, 128, 3)['seventy_objects']
    y_pred = _seeded_y_pred(case._replace(y_true=bc.empty_y_true(2, 160, 128, 3)), 12, seed=1)
    with pytest.raises(ValueError, match='gt_cap'):
        eval_utils.evaluate_on_device(y_pred, case.y_true, 3, gt_cap=8)
    tp, true, pred = eval_utils.evaluate_on_device(y_pred, case.y_true, 3, calc_now=False, gt_cap=70)
    assert sum(true.values()) == 80
