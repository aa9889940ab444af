# coding: utf-8
"""Evaluation bookkeeping of the reference (utils/eval_utils.py) on top of the device-resident detection path —
SURVEY.md §8(f) row 2.  Same function names, argument order and return values as the reference:

  calc_iou            utils/eval_utils.py:13-46     IoU matrix [N,V] (numpy, float64 in / float64 out)
  evaluate_on_cpu     utils/eval_utils.py:49-139    recall / precision of one batch, NMS = cpu_nms semantics
  evaluate_on_gpu     utils/eval_utils.py:142-232   same with the gpu_nms op
  evaluate_on_device  (same rule)                   the batch at once on the device (y3_batch_eval), one table back
  get_preds_gpu       utils/eval_utils.py:235-261   [[image_id, x_min, y_min, x_max, y_max, score, label], ...]
  parse_gt_rec        utils/eval_utils.py:264-307   annotation file -> {img_id: [[x0, y0, x1, y1, label], ...]}
  voc_ap, voc_eval    utils/eval_utils.py:312-423   PASCAL VOC AP (area and 11-point) per class
  coco_eval           (beyond the reference)        COCO bbox metrics: AP@[.50:.95], AP50, AP75, AP / AR by size, AR@1/10/100

plus `get_preds_batch`, the MI355X-first form: N images per call, detections produced by `yolov3.detect`
(forward -> decode -> batched per-class NMS on the device, one host transfer per batch instead of two
`sess.run` round trips per image).

The TF plumbing arguments of the reference signatures (`sess`, `pred_boxes_flag`, `pred_scores_flag`) are kept
positionally and ignored; `gpu_nms_op` is a callable `(boxes [1,B,4], scores [1,B,C]) -> (boxes, scores, labels)`
(default: utils.nms_utils.gpu_nms with the arguments bound by the caller).

All arithmetic that decides a match or an AP value is done in float64 numpy in the reference's operation order, so
the results are bit-identical to the reference's (pinned by tests/golden/reference_eval_goldens.npz).
"""
from __future__ import division, print_function

import numpy as np

from .data_utils import parse_line
from .nms_utils import cpu_nms


def _to_numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def calc_iou(pred_boxes, true_boxes):
    '''
    IoU matrix via numpy broadcasting.
    shape_info: pred_boxes: [N, 4] (x_min, y_min, x_max, y_max)
                true_boxes: [V, 4]
    return: IoU matrix: shape: [N, V]
    '''
    p = np.asarray(pred_boxes)[:, None, :]        # [N, 1, 4]
    t = np.asarray(true_boxes)[None, :, :]        # [1, V, 4]
    wh = np.maximum(np.minimum(p[..., 2:], t[..., 2:]) - np.maximum(p[..., :2], t[..., :2]), 0.)
    inter = wh[..., 0] * wh[..., 1]
    p_wh = p[..., 2:] - p[..., :2]
    t_wh = t[..., 2:] - t[..., :2]
    p_area = p_wh[..., 0] * p_wh[..., 1]
    t_area = t_wh[..., 0] * t_wh[..., 1]
    return inter / (p_area + t_area - inter + 1e-10)


def _ground_truth_of_image(y_true, i):
    """Labels [V] and corner boxes [V,4] of image i, gathered over the three y_true scales in the reference's
    order (scale 13 first, row-major inside a scale)."""
    labels, boxes = [], []
    for j in range(3):
        yt = _to_numpy(y_true[j][i])
        probs = yt[..., 5:-1]
        mask = probs.sum(axis=-1) > 0
        labels.append(np.argmax(probs[mask], axis=-1))
        boxes.append(yt[..., 0:4][mask])
    labels = np.concatenate(labels)
    centre_wh = np.concatenate(boxes).astype(np.float64)   # the reference round-trips through python floats
    corners = np.empty_like(centre_wh)
    corners[:, 0:2] = centre_wh[:, 0:2] - centre_wh[:, 2:4] / 2.
    corners[:, 2:4] = corners[:, 0:2] + centre_wh[:, 2:4]
    return labels, corners


def _evaluate(y_pred, y_true, num_classes, nms_fn, iou_thresh, calc_now):
    """Shared body of evaluate_on_cpu / evaluate_on_gpu.  A ground-truth object counts as found when at least one
    detection has it as its best-IoU object with IoU > iou_thresh and the same label (the reference's
    confidence-replacement loop never changes WHICH objects are matched, only which detection is credited)."""
    num_images = y_true[0].shape[0]
    n_true = np.zeros(num_classes, np.int64)
    n_pred = np.zeros(num_classes, np.int64)
    n_tp = np.zeros(num_classes, np.int64)
    boxes_all, confs_all, probs_all = (_to_numpy(t) for t in y_pred)
    for i in range(num_images):
        gt_labels, gt_boxes = _ground_truth_of_image(y_true, i)
        n_true += np.bincount(gt_labels, minlength=num_classes)[:num_classes]
        det_boxes, _, det_labels = nms_fn(boxes_all[i:i + 1], confs_all[i:i + 1] * probs_all[i:i + 1])
        if det_labels is None or len(det_labels) == 0:
            continue
        det_boxes, det_labels = _to_numpy(det_boxes), _to_numpy(det_labels).astype(np.int64)
        n_pred += np.bincount(det_labels, minlength=num_classes)[:num_classes]
        if gt_labels.size == 0:
            continue                      # (the reference indexes an empty array here and raises)
        iou = calc_iou(det_boxes, gt_boxes)
        best = np.argmax(iou, axis=-1)
        hit = (iou[np.arange(len(best)), best] > iou_thresh) & (gt_labels[best] == det_labels)
        found = np.unique(best[hit])
        n_tp += np.bincount(gt_labels[found], minlength=num_classes)[:num_classes]
    if calc_now:
        # avoid divided by 0
        return n_tp.sum() / (n_true.sum() + 1e-6), n_tp.sum() / (n_pred.sum() + 1e-6)
    as_dict = lambda a: {c: int(a[c]) for c in range(num_classes)}
    return as_dict(n_tp), as_dict(n_true), as_dict(n_pred)


def evaluate_on_cpu(y_pred, y_true, num_classes, calc_now=True, max_boxes=50, score_thresh=0.5, iou_thresh=0.5):
    '''
    Given y_pred (boxes [N,B,4], confs [N,B,1], probs [N,B,C]) and y_true (the three process_box tensors) of a
    batch, get the recall and precision of the batch (calc_now) or the per-class
    (true_positive_dict, true_labels_dict, pred_labels_dict).  NMS follows cpu_nms (utils/nms_utils.py:94-123).
    '''
    nms = lambda b, s: cpu_nms(b, s, num_classes, max_boxes=max_boxes, score_thresh=score_thresh,
                               iou_thresh=iou_thresh)
    return _evaluate(y_pred, y_true, num_classes, nms, iou_thresh, calc_now)


def evaluate_on_gpu(sess, gpu_nms_op, pred_boxes_flag, pred_scores_flag, y_pred, y_true, num_classes, iou_thresh=0.5,
                    calc_now=True):
    '''
    Same as evaluate_on_cpu with the NMS given by `gpu_nms_op` (a callable (boxes, scores) -> (boxes, scores,
    labels), e.g. functools.partial(gpu_nms, num_classes=C, max_boxes=.., score_thresh=.., nms_thresh=..)).
    `sess`, `pred_boxes_flag`, `pred_scores_flag` exist for signature compatibility and are ignored.
    '''
    return _evaluate(y_pred, y_true, num_classes, gpu_nms_op, iou_thresh, calc_now)


def batch_eval_counts(detections, y_true, num_classes, iou_thresh=0.5, gt_cap=None, table=None):
    """y3_batch_eval (include/yolo355.h) on device tensors: `detections` is what gpu_nms_batched(..., lazy=True) returned, or
    its (boxes [n,cap,4] f32, scores, labels [n,cap] i32, counts [n] i32) device tensors; y_true the batch's three
    process_box tensors.  Returns the int64 device tensor [num_classes + 1, 3]: rows (n_tp, n_true, n_pred) per class, and in
    row num_classes, column 0, the number of objects dropped for lack of gt_cap.  `table`: such a tensor to add to
    (several batches in one table).  Nothing waits for the host."""
    import ctypes
    import torch
    from .. import _lib, framework as fw
    ob, _, ol, cnt = detections.device_tensors() if hasattr(detections, 'device_tensors') else detections
    yt = [fw.as_device_f32(t) for t in y_true]
    n, cap, C = int(ob.shape[0]), int(ob.shape[1]), int(num_classes)
    if len(yt) != 3 or any(t.dim() != 5 or int(t.shape[0]) != n or int(t.shape[3]) != 3 or int(t.shape[4]) != C + 6 for t in yt):
        raise ValueError("batch_eval_counts: y_true must be three [%d, g, g, 3, %d] tensors, got %s" % (
            n, C + 6, [tuple(t.shape) for t in yt]))
    h, w = 32 * int(yt[0].shape[1]), 32 * int(yt[0].shape[2])
    if [tuple(t.shape[1:3]) for t in yt] != [(h // 32, w // 32), (h // 16, w // 16), (h // 8, w // 8)]:
        raise ValueError("batch_eval_counts: y_true grids %s are not those of one input size" % [tuple(t.shape[1:3]) for t in yt])
    if ob.dtype != torch.float32 or ol.dtype != torch.int32 or cnt.dtype != torch.int32 or tuple(ol.shape) != (n, cap) \
            or tuple(cnt.shape) != (n,):
        raise ValueError("batch_eval_counts: detections must be fp32 boxes [n,cap,4], int32 labels [n,cap] and counts [n]")
    dev = ob.device
    if gt_cap is None:
        gt_cap = min(sum(int(t.shape[1]) * int(t.shape[2]) * 3 for t in yt), 4096)
    gt_cap = int(gt_cap)
    L = _lib.lib()
    nbytes = L.y3_batch_eval_scratch_bytes(n, gt_cap)
    if nbytes == 0:
        raise ValueError("batch_eval_counts: non-positive dimension (n=%d, gt_cap=%d)" % (n, gt_cap))
    ws = fw.stream_scratch('batch_eval', dev, nbytes)
    if table is None:
        table = torch.zeros((C + 1, 3), dtype=torch.int64, device=dev)
    ob, ol, cnt = ob.contiguous(), ol.contiguous(), cnt.contiguous()
    state = table[C].view(torch.int32)      # the overflow word: the first 4 bytes of the row behind the classes
    _lib.check(L.y3_batch_eval(fw.context(dev), fw.ptr(ob), fw.ptr(ol), fw.ptr(cnt), n, cap, fw.ptr(yt[0]), fw.ptr(yt[1]),
                               fw.ptr(yt[2]), h, w, C, ctypes.c_double(iou_thresh), gt_cap, fw.ptr(ws), ctypes.c_size_t(nbytes),
                               fw.ptr(table), fw.ptr(state)))
    return table


def evaluate_on_device(y_pred, y_true, num_classes, max_boxes=50, score_thresh=0.5, nms_thresh=0.5, iou_thresh=0.5,
                       calc_now=True, gt_cap=None):
    '''
    evaluate_on_gpu with the whole batch kept on the device: one gpu_nms_batched call, then y3_batch_eval
    (include/yolo355.h) gathers the ground truth out of y_true, matches and counts; one [num_classes + 1, 3] integer table
    comes back.  y_pred: (boxes, confs, probs) as yolov3.predict returns them, or (boxes, scores) with scores = confs * probs
    (predict(..., with_scores=True)).  Returns what evaluate_on_gpu returns for
    gpu_nms_op = functools.partial(gpu_nms, num_classes=.., max_boxes=.., score_thresh=.., nms_thresh=..).
    gt_cap: objects kept per image (default: the image's cell count, at most 4096); ValueError when an image has more.
    Precondition: y_true's class entries are finite and >= 0 (csrc/y3_beval_px.h).
    '''
    from .. import framework as fw
    from .nms_utils import gpu_nms_batched
    if len(y_pred) == 2:
        boxes, scores = y_pred
    else:
        boxes, confs, probs = y_pred
        scores = fw.as_device_f32(confs) * fw.as_device_f32(probs)
    dets = gpu_nms_batched(boxes, scores, num_classes, max_boxes, score_thresh, nms_thresh, lazy=True)
    table = batch_eval_counts(dets, y_true, num_classes, iou_thresh, gt_cap).cpu().numpy()      # the one transfer
    fw.check_context(dets.device_tensors()[0].device)
    dropped = int(table[num_classes, 0] & 0xFFFFFFFF)
    if dropped:
        raise ValueError("evaluate_on_device: %d objects did not fit gt_cap: raise gt_cap" % dropped)
    n_tp, n_true, n_pred = table[:num_classes, 0], table[:num_classes, 1], table[:num_classes, 2]
    if calc_now:
        # avoid divided by 0
        return n_tp.sum() / (n_true.sum() + 1e-6), n_tp.sum() / (n_pred.sum() + 1e-6)
    as_dict = lambda a: {c: int(a[c]) for c in range(num_classes)}
    return as_dict(n_tp), as_dict(n_true), as_dict(n_pred)


def _rows(image_id, boxes, scores, labels):
    boxes, scores, labels = _to_numpy(boxes), _to_numpy(scores), _to_numpy(labels)
    return [[image_id, boxes[k][0], boxes[k][1], boxes[k][2], boxes[k][3], scores[k], labels[k]]
            for k in range(len(labels))]


def get_preds_gpu(sess, gpu_nms_op, pred_boxes_flag, pred_scores_flag, image_ids, y_pred):
    '''
    Given the y_pred of ONE input image, get the predicted bbox and label info.
    return:
        pred_content: 2d list, rows [image_id, x_min, y_min, x_max, y_max, score, label].
    '''
    boxes, confs, probs = y_pred[0][0:1], y_pred[1][0:1], y_pred[2][0:1]
    det = gpu_nms_op(boxes, confs * probs)
    return _rows(image_ids[0], *det)


def get_preds_batch(image_ids, detections):
    """Rows of get_preds_gpu for a whole batch: `detections` is the list yolov3.detect returns (one
    (boxes, scores, labels) tuple of device tensors per image)."""
    out = []
    for image_id, det in zip(image_ids, detections):
        out += _rows(image_id, *det)
    return out


gt_dict = {}  # key: img_id, value: gt object list (module-level cache, like the reference)


def parse_gt_rec(gt_filename, target_img_size, letterbox_resize=True):
    '''
    parse and re-organize the gt info: boxes are mapped to the network input frame
    (letterbox: scale by min ratio + integer pad; else independent x/y scale).
    return:
        gt_dict: dict. Each key is a img_id, the value is the gt bboxes in the corresponding img.
    '''
    global gt_dict
    if gt_dict:
        return gt_dict
    new_width, new_height = target_img_size
    with open(gt_filename, 'r') as f:
        for line in f:
            img_id, _, boxes, labels, ori_width, ori_height = parse_line(line)
            if letterbox_resize:
                ratio = min(new_width / ori_width, new_height / ori_height)
                sx = sy = ratio
                dw = int((new_width - int(ratio * ori_width)) / 2)
                dh = int((new_height - int(ratio * ori_height)) / 2)
            else:
                sx, sy, dw, dh = None, None, 0, 0
            objects = []
            for (x_min, y_min, x_max, y_max), label in zip(boxes, labels):
                if letterbox_resize:
                    objects.append([x_min * sx + dw, y_min * sy + dh, x_max * sx + dw, y_max * sy + dh, label])
                else:
                    objects.append([x_min * new_width / ori_width, y_min * new_height / ori_height,
                                    x_max * new_width / ori_width, y_max * new_height / ori_height, label])
            gt_dict[img_id] = objects
    return gt_dict


def voc_ap(rec, prec, use_07_metric=False):
    """VOC AP from cumulative recall / precision arrays: the 11-point VOC07 metric, or (default) the area under
    the monotone precision envelope."""
    rec, prec = np.asarray(rec), np.asarray(prec)
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            above = rec >= t
            ap = ap + (np.max(prec[above]) if above.any() else 0) / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]          # precision envelope (running max from the right)
    step = np.where(mrec[1:] != mrec[:-1])[0]                # where recall changes value
    return np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1])


def voc_eval(gt_dict, val_preds, classidx, iou_thres=0.5, use_07_metric=False):
    '''
    PASCAL VOC evaluation of one class.
    gt_dict: parse_gt_rec's dict; val_preds: rows of get_preds_gpu over the whole set.
    returns (npos, nd, recall, precision, ap); (1e-6, 1e-6, 0, 0, 0) when the class has no detection.
    '''
    gt_boxes, gt_used, npos = {}, {}, 0
    for img_id, objs in gt_dict.items():
        mine = np.array([o[:4] for o in objs if o[-1] == classidx], dtype=np.float64).reshape(-1, 4)
        gt_boxes[img_id] = mine
        gt_used[img_id] = np.zeros(len(mine), bool)
        npos += len(mine)

    pred = [p for p in val_preds if p[-1] == classidx]
    if not pred:
        print('no box, ignore')
        return 1e-6, 1e-6, 0, 0, 0
    order = np.argsort(-np.array([p[-2] for p in pred]))      # by descending confidence
    nd = len(pred)
    tp = np.zeros(nd)
    for rank, k in enumerate(order):
        img_id = pred[k][0]
        bb = np.array(pred[k][1:5], dtype=np.float64)
        g = gt_boxes[img_id]
        if g.size == 0:
            continue
        # pixel-inclusive (+1) intersection over union, as in the VOC devkit
        iw = np.maximum(np.minimum(g[:, 2], bb[2]) - np.maximum(g[:, 0], bb[0]) + 1., 0.)
        ih = np.maximum(np.minimum(g[:, 3], bb[3]) - np.maximum(g[:, 1], bb[1]) + 1., 0.)
        inters = iw * ih
        uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.)
               - inters)
        overlaps = inters / uni
        j = int(np.argmax(overlaps))
        if overlaps[j] > iou_thres and not gt_used[img_id][j]:
            gt_used[img_id][j] = True          # first (most confident) detection of this object
            tp[rank] = 1.
    fp = np.cumsum(1. - tp)
    tp = np.cumsum(tp)
    rec = tp / float(npos)
    # avoid divide by zero in case the first detection matches a difficult ground truth
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    ap = voc_ap(rec, prec, use_07_metric)
    return npos, nd, tp[-1] / float(npos), tp[-1] / float(nd), ap


COCO_IOU_THRS = np.linspace(.5, .95, 10)          # (the ninth is 0.8999999999999999: the kernels take them from here)
COCO_REC_THRS = np.linspace(0., 1., 101)
COCO_AREA_RANGES = ((0., 1e10), (0., 32. ** 2), (32. ** 2, 96. ** 2), (96. ** 2, 1e10))      # all, small, medium, large
COCO_MAX_DETS = (1, 10, 100)
COCO_STAT_NAMES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl')


def parse_gt_area_scale(gt_filename, target_img_size, letterbox_resize=True):
    """{img_id: 1 / (sx * sy)} for parse_gt_rec's mapping of the same annotation lines: the factor that turns an area in the
    network-input frame back into original pixels, so that coco_eval's small / medium / large are COCO's."""
    new_width, new_height = target_img_size
    out = {}
    with open(gt_filename, 'r') as f:
        for line in f:
            img_id, _, _, _, ori_width, ori_height = parse_line(line)
            if letterbox_resize:
                sx = sy = min(new_width / ori_width, new_height / ori_height)
            else:
                sx, sy = new_width / ori_width, new_height / ori_height
            out[img_id] = 1. / (sx * sy)
    return out


def _coco_mean(values):
    values = np.asarray(values, np.float64)
    values = values[values > -1]
    return float(np.mean(values)) if values.size else -1.


def _coco_twelve(precision, recall):
    """The twelve numbers of precision [T,R,K',A,M] / recall [T,K',A,M] (K' = all classes, or one)."""
    out = [_coco_mean(precision[:, :, :, 0, 2]), _coco_mean(precision[0, :, :, 0, 2]), _coco_mean(precision[5, :, :, 0, 2])]
    out += [_coco_mean(precision[:, :, :, a, 2]) for a in (1, 2, 3)]
    out += [_coco_mean(recall[:, :, 0, m]) for m in (0, 1, 2)]
    out += [_coco_mean(recall[:, :, a, 2]) for a in (1, 2, 3)]
    return np.array(out, np.float64)


def coco_eval(gt_dict, val_preds, class_num, area_scale=None):
    """
    COCO bbox evaluation (the COCOeval rule, no crowd objects: the annotation format has none) of all classes.
    gt_dict: parse_gt_rec's dict, whose order is the image order; val_preds: rows of get_preds_batch over the whole set;
    area_scale: {img_id: factor} an object's or detection's area is multiplied by before the area-range test
    (parse_gt_area_scale; default 1.0).
    returns {'precision': f64 [10, 101, K, 4, 3], 'recall': f64 [10, K, 4, 3], 'stats': f64 [12], 'per_class': f64 [K, 12]}
    (IoU threshold, recall threshold, class, area range all/small/medium/large, max-dets 1/10/100); stats and per_class are
    COCO_STAT_NAMES, -1 where nothing is defined.  The rule is written out in include/yolo355.h (y3_coco_match).
    """
    K, T, R, A, M = int(class_num), len(COCO_IOU_THRS), len(COCO_REC_THRS), len(COCO_AREA_RANGES), len(COCO_MAX_DETS)
    eps = np.spacing(1)
    image_ids = list(gt_dict)
    index = {img_id: i for i, img_id in enumerate(image_ids)}
    scale = np.array([1. if area_scale is None else float(area_scale[i]) for i in image_ids], np.float64)

    def outside(boxes, factor):      # [n, A] bool: the area is outside the range
        ar = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) * factor
        return np.stack([(ar < lo) | (ar > hi) for lo, hi in COCO_AREA_RANGES], axis=1).reshape(-1, A)

    # objects per (image, class) in ground-truth order, and the objects inside each range per class
    gts, npig = {}, np.zeros((K, A), np.int64)
    for img_id, objs in gt_dict.items():
        for o in objs:
            gts.setdefault((index[img_id], int(o[-1])), []).append([float(v) for v in o[:4]])
    for (im, k), boxes in gts.items():
        gts[(im, k)] = boxes = np.array(boxes, np.float64).reshape(-1, 4)
        if 0 <= k < K:
            npig[k] += (~outside(boxes, scale[im])).sum(axis=0)

    # detections by (image, label, score descending, arrival)
    P = len(val_preds)
    d_img = np.array([index[p[0]] for p in val_preds], np.int64).reshape(P)
    d_box = np.array([[float(v) for v in p[1:5]] for p in val_preds], np.float64).reshape(P, 4)
    d_score = np.array([float(p[5]) for p in val_preds], np.float64).reshape(P)
    d_label = np.array([int(p[6]) for p in val_preds], np.int64).reshape(P)
    order = np.lexsort((np.arange(P), -d_score, d_label, d_img))
    d_img, d_box, d_score, d_label = d_img[order], d_box[order], d_score[order], d_label[order]
    key = d_img * max(K, 1) + d_label
    heads = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if P else np.zeros(0, np.int64)
    ends = np.concatenate((heads[1:], [P])).astype(np.int64)
    grank = np.zeros(P, np.int64)
    matched = np.zeros((P, T, A), bool)
    ignored = np.zeros((P, T, A), bool)
    for h, e in zip(heads, ends):
        grank[h:e] = np.arange(e - h)
        D = min(e - h, COCO_MAX_DETS[-1])
        im, k = int(d_img[h]), int(d_label[h])
        det = d_box[h:h + D]
        d_out = outside(det, scale[im])
        g = gts.get((im, k))
        if g is None:
            ignored[h:h + D] = d_out[:, None, :]
            continue
        G = len(g)
        w = np.minimum(det[:, None, 2], g[None, :, 2]) - np.maximum(det[:, None, 0], g[None, :, 0])
        hh = np.minimum(det[:, None, 3], g[None, :, 3]) - np.maximum(det[:, None, 1], g[None, :, 1])
        inter = w * hh
        with np.errstate(all='ignore'):
            ious = inter / (((det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1]))[:, None]
                            + ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[None, :] - inter)
        ious = np.where((w <= 0.) | (hh <= 0.), 0., ious).tolist()
        g_out = outside(g, scale[im])
        for a in range(A):
            g_ig = g_out[:, a].tolist()
            for ti, t in enumerate(COCO_IOU_THRS):
                taken = [False] * G
                floor = min(float(t), 1 - 1e-10)
                for d in range(D):
                    row, best, m = ious[d], floor, -1
                    for j in range(G):                  # the objects that count
                        if g_ig[j] or taken[j] or row[j] < best:
                            continue
                        best, m = row[j], j
                    if m < 0:
                        for j in range(G):              # only then the ignored ones
                            if not g_ig[j] or taken[j] or row[j] < best:
                                continue
                            best, m = row[j], j
                    if m >= 0:
                        taken[m] = True
                        matched[h + d, ti, a] = True
                        ignored[h + d, ti, a] = g_ig[m]
                    else:
                        ignored[h + d, ti, a] = d_out[d, a]

    precision = -np.ones((T, R, K, A, M), np.float64)
    recall = -np.ones((T, K, A, M), np.float64)
    for k in range(K):
        of_class = np.flatnonzero(d_label == k)          # image ascending, in-group rank ascending
        for mi, max_det in enumerate(COCO_MAX_DETS):
            sel = of_class[grank[of_class] < max_det]
            sel = sel[np.argsort(-d_score[sel], kind='mergesort')]
            for a in range(A):
                if npig[k, a] == 0:
                    continue
                dm, dig = matched[sel][:, :, a], ignored[sel][:, :, a]
                tps = np.cumsum(dm & ~dig, axis=0).astype(np.float64)
                fps = np.cumsum(~dm & ~dig, axis=0).astype(np.float64)
                for ti in range(T):
                    tp, fp = tps[:, ti], fps[:, ti]
                    nd = len(tp)
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + eps)
                    recall[ti, k, a, mi] = rc[-1] if nd else 0.
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    at = np.searchsorted(rc, COCO_REC_THRS, side='left')
                    q = np.zeros(R)
                    q[at < nd] = pr[at[at < nd]]
                    precision[ti, :, k, a, mi] = q
    per_class = np.stack([_coco_twelve(precision[:, :, k:k + 1], recall[:, k:k + 1]) for k in range(K)]).reshape(K, 12)
    return {'precision': precision, 'recall': recall, 'stats': _coco_twelve(precision, recall), 'per_class': per_class}


def coco_summary_lines(stats):
    """The twelve report lines of coco_eval's / DeviceEval.finish_coco's `stats`, in COCOeval's layout."""
    rows = [('Average Precision', '(AP)', '0.50:0.95', 'all', 100), ('Average Precision', '(AP)', '0.50', 'all', 100),
            ('Average Precision', '(AP)', '0.75', 'all', 100), ('Average Precision', '(AP)', '0.50:0.95', 'small', 100),
            ('Average Precision', '(AP)', '0.50:0.95', 'medium', 100), ('Average Precision', '(AP)', '0.50:0.95', 'large', 100),
            ('Average Recall', '(AR)', '0.50:0.95', 'all', 1), ('Average Recall', '(AR)', '0.50:0.95', 'all', 10),
            ('Average Recall', '(AR)', '0.50:0.95', 'all', 100), ('Average Recall', '(AR)', '0.50:0.95', 'small', 100),
            ('Average Recall', '(AR)', '0.50:0.95', 'medium', 100), ('Average Recall', '(AR)', '0.50:0.95', 'large', 100)]
    return ['{:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(title, kind, iou, area, dets, float(v))
            for (title, kind, iou, area, dets), v in zip(rows, stats)]


class DeviceEval(object):
    """voc_eval for every class at once on the device (y3_voc_append / y3_voc_match / y3_voc_ap, include/yolo355.h):
    the detections stay where the NMS kernels left them, and one [class_num, 5] table comes back.

        ev = DeviceEval(gt_dict, image_ids, class_num)
        ev.add(batch_image_ids, gpu_nms_batched(..., lazy=True))      # per batch; nothing waits for the host
        table = ev.finish(iou_thres=0.5, use_07_metric=False)         # rows (npos, nd, recall, precision, ap)
        coco = ev.finish_coco(area_scale)                             # coco_eval's 'stats' and 'per_class' (either order)

    A row of the table is what voc_eval(gt_dict, val_preds, c, iou_thres, use_07_metric) returns for the rows
    get_preds_batch would have built, with two differences in the last bits' provenance:
      - order: voc_eval ranks with np.argsort(-score), whose default sort is not stable; here the rank order is stable -
        descending score, then ascending row in arrival (append) order.  For distinct scores within a class the two orders
        are the same order;
      - the area AP is summed in a fixed order of its own, so it lies within nd * 2**-52 of voc_ap's np.sum (pairwise);
        npos, nd, recall, precision and the 11-point AP are the same float64 values.
    Matching arithmetic is float64 on the device in voc_eval's operation order; ground-truth boxes stay float64 (parse_gt_rec's
    letterboxed values are not fp32 numbers), detection boxes and scores are the NMS kernel's fp32 values widened exactly.
    The table is bit-identical from run to run.

    gt_dict: parse_gt_rec's dict.  image_ids: the ids of the set, each a key of gt_dict (ValueError otherwise); their order
    fixes the image index inside the arena.  capacity_rows: detections the arena holds (48 bytes each; default 1,024 per
    image); finish raises when more were added.  arena: caller-owned (box f64 [R,4], score f64 [R], label i32 [R],
    image i32 [R]) device tensors to use instead of allocating them.
    """

    def __init__(self, gt_dict, image_ids, class_num, capacity_rows=None, arena=None, device=None):
        import torch
        from .. import framework as fw
        self.class_num = int(class_num)
        if self.class_num <= 0:
            raise ValueError("DeviceEval: class_num must be positive")
        self._index, starts, boxes, labels = {}, [0], [], []
        for img_id in image_ids:
            if img_id not in gt_dict:
                raise ValueError("DeviceEval: image id %r is not in gt_dict" % (img_id,))
            if img_id in self._index:
                raise ValueError("DeviceEval: image id %r is listed twice" % (img_id,))
            self._index[img_id] = len(self._index)
            for obj in gt_dict[img_id]:
                boxes.append([float(v) for v in obj[:4]])
                labels.append(int(obj[-1]) if obj[-1] == int(obj[-1]) else -1)
            starts.append(len(labels))
        if not self._index:
            raise ValueError("DeviceEval: no image")
        self.num_gt = len(labels)
        self._dev = torch.device(device) if device is not None else fw.default_device()
        to_dev = lambda a: torch.from_numpy(a).to(self._dev)
        self._gt_start = to_dev(np.asarray(starts, np.int32))
        self._gt_box = to_dev(np.asarray(boxes or [[0.] * 4], np.float64).reshape(-1, 4))
        self._gt_label = to_dev(np.asarray(labels or [-1], np.int32))
        R = int(capacity_rows) if capacity_rows is not None else 1024 * len(self._index)
        if not 0 < R < 2 ** 31:
            raise ValueError("DeviceEval: capacity_rows must be in 1 .. 2**31 - 1")
        self.capacity_rows = R
        if arena is None:
            arena = (torch.zeros((R, 4), dtype=torch.float64, device=self._dev), torch.zeros(R, dtype=torch.float64, device=self._dev),
                     torch.zeros(R, dtype=torch.int32, device=self._dev), torch.zeros(R, dtype=torch.int32, device=self._dev))
        for t, dtype, shape in zip(arena, (torch.float64, torch.float64, torch.int32, torch.int32), ((R, 4), (R,), (R,), (R,))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device.type != 'cuda':
                raise ValueError("DeviceEval: arena tensors must be contiguous device tensors f64 [R,4], f64 [R], i32 [R], i32 [R]")
        self._arena = tuple(arena)
        self._state = torch.zeros(2, dtype=torch.int32, device=self._dev)        # rows in the arena, rows that did not fit

    def _indices(self, image_ids_of_batch):
        try:
            return [self._index[i] for i in image_ids_of_batch]
        except KeyError as e:
            raise ValueError("DeviceEval: image id %r is not in gt_dict" % (e.args[0],))

    def add(self, image_ids_of_batch, detections):
        """Append one batch: `detections` is what gpu_nms_batched(..., lazy=True) / yolov3.detect returned (it is not
        materialised), or the (boxes [n,cap,4], scores [n,cap], labels [n,cap], counts [n]) device tensors themselves."""
        import torch
        from .. import _lib, framework as fw
        ob, osc, ol, cnt = detections.device_tensors() if hasattr(detections, 'device_tensors') else detections
        n, cap = int(ob.shape[0]), int(ob.shape[1])
        idx = self._indices(image_ids_of_batch)
        if len(idx) != n or tuple(osc.shape) != (n, cap) or tuple(ol.shape) != (n, cap) or tuple(cnt.shape) != (n,):
            raise ValueError("DeviceEval.add: %d image ids for detections of shapes %s %s %s %s" % (
                len(idx), tuple(ob.shape), tuple(osc.shape), tuple(ol.shape), tuple(cnt.shape)))
        if ob.dtype != torch.float32 or osc.dtype != torch.float32 or ol.dtype != torch.int32 or cnt.dtype != torch.int32:
            raise ValueError("DeviceEval.add: detections must be fp32 boxes and scores, int32 labels and counts")
        img = torch.tensor(idx, dtype=torch.int32).pin_memory().to(self._dev, non_blocking=True)
        box, score, label, image = self._arena
        _lib.check(_lib.lib().y3_voc_append(fw.context(self._dev), fw.ptr(ob), fw.ptr(osc), fw.ptr(ol), fw.ptr(cnt), fw.ptr(img), n,
                                            cap, fw.ptr(box), fw.ptr(score), fw.ptr(label), fw.ptr(image), self.capacity_rows,
                                            fw.ptr(self._state)))

    def add_rows(self, image_ids, boxes, scores, labels):
        """Append rows that are already on the host as float64 (one image id per row): the route of stored reference vectors,
        whose boxes and scores are not fp32 numbers.  Plumbing only; synchronises."""
        import torch
        k = len(image_ids)
        at = int(self._state[0].item())
        if at + k > self.capacity_rows:
            raise ValueError("DeviceEval.add_rows: %d rows do not fit behind %d of %d" % (k, at, self.capacity_rows))
        box, score, label, image = self._arena
        box[at:at + k] = torch.from_numpy(np.asarray(boxes, np.float64).reshape(k, 4)).to(self._dev)
        score[at:at + k] = torch.from_numpy(np.asarray(scores, np.float64).reshape(k)).to(self._dev)
        label[at:at + k] = torch.from_numpy(np.asarray(labels, np.int32).reshape(k)).to(self._dev)
        image[at:at + k] = torch.from_numpy(np.asarray(self._indices(image_ids), np.int32)).to(self._dev)
        self._state[0] += k

    def _rank(self, *keys):
        """Plumbing: the int32 order of the arena's rows (or of their ranks) by stable sorts, the last key first.  Each key is
        (tensor [R], fill): rows at or past the arena's count take `fill` (None: the value as it is), which ranks them behind
        every detection."""
        import torch
        live = torch.arange(self.capacity_rows, device=self._dev, dtype=torch.int32) < self._state[0]
        order = None
        for key, fill in keys:
            if fill is not None:
                key = torch.where(live, key, torch.full_like(key, fill))
            order = torch.sort(key, stable=True).indices if order is None else order[torch.sort(key[order], stable=True).indices]
        return order.to(torch.int32).contiguous()

    def _read_back(self, out, at, upto):
        """out[:upto] on the host, with the arena's two counters in out[at:at + 2]: the one device -> host copy of a finish.
        Raises Y3Error when rows were dropped for lack of capacity."""
        import torch
        from .. import _lib, framework as fw
        out[at:at + 2] = self._state.to(torch.float64)
        host = out[:upto].cpu().numpy()
        fw.check_context(self._dev)
        rows, lost = int(host[at]), int(host[at + 1])
        if lost:
            raise _lib.Y3Error("DeviceEval: %d detections did not fit the arena's %d rows (%d kept): raise capacity_rows" % (
                lost, self.capacity_rows, rows))
        return host

    def finish(self, iou_thres=0.5, use_07_metric=False):
        """The [class_num, 5] float64 table of (npos, nd, recall, precision, ap).  One device -> host copy (the table with the
        arena's two counters behind it); raises Y3Error when rows were dropped for lack of capacity."""
        import ctypes
        import torch
        from .. import _lib, framework as fw
        L, ctx, dev, R, C = _lib.lib(), fw.context(self._dev), self._dev, self.capacity_rows, self.class_num
        box, score, label, image = self._arena
        # rank order: label ascending, score descending, row ascending.  Negating a float64 is exact.
        order = self._rank((-score, None), (label, C))
        m_bytes, a_bytes = L.y3_voc_match_scratch_bytes(R, self.num_gt), L.y3_voc_ap_scratch_bytes(R)
        scratch = torch.empty(max(m_bytes, a_bytes), dtype=torch.uint8, device=dev)
        tp = torch.empty(R, dtype=torch.uint8, device=dev)
        seg = torch.empty(C + 1, dtype=torch.int32, device=dev)
        out = torch.zeros(5 * C + 2, dtype=torch.float64, device=dev)
        _lib.check(L.y3_voc_match(ctx, fw.ptr(box), fw.ptr(label), fw.ptr(image), fw.ptr(order), R, fw.ptr(self._state),
                                  fw.ptr(self._gt_start), fw.ptr(self._gt_box), fw.ptr(self._gt_label), len(self._index),
                                  self.num_gt, C, ctypes.c_double(iou_thres), fw.ptr(scratch), ctypes.c_size_t(m_bytes), fw.ptr(tp),
                                  fw.ptr(seg)))
        thresholds = (ctypes.c_double * 11)(*np.arange(0., 1.1, 0.1))
        _lib.check(L.y3_voc_ap(ctx, fw.ptr(tp), fw.ptr(seg), R, fw.ptr(self._gt_label), self.num_gt, C, int(bool(use_07_metric)),
                               thresholds, fw.ptr(scratch), ctypes.c_size_t(a_bytes), fw.ptr(out)))
        return self._read_back(out, 5 * C, 5 * C + 2)[:5 * C].reshape(C, 5).copy()

    def finish_coco(self, area_scale=None, return_curves=False):
        """coco_eval's numbers for the rows in the arena (y3_coco_match / y3_coco_ap / y3_coco_summary, include/yolo355.h):
        {'stats': f64 [12], 'per_class': f64 [class_num, 12]}, and with return_curves also 'precision' [10, 101, class_num, 4, 3]
        and 'recall' [10, class_num, 4, 3].  area_scale: {img_id: factor} as coco_eval takes it (default 1.0).  precision and
        recall are coco_eval's float64 values bit for bit (its image order = this evaluator's image_ids order); stats and
        per_class are summed in a fixed order of their own, within n * 2**-52 of numpy's mean over n entries, and are the same
        bits in every run.  One device -> host copy (the numbers with the arena's two counters behind them); raises Y3Error when
        rows were dropped for lack of capacity.  `finish` and `finish_coco` read the arena and leave it as it is."""
        import ctypes
        import torch
        from .. import _lib, framework as fw
        L, ctx, dev, R, C = _lib.lib(), fw.context(self._dev), self._dev, self.capacity_rows, self.class_num
        N = len(self._index)
        box, score, label, image = self._arena
        # order: (image, label, score descending, row).  order2 sorts the RANKS of order by (label, score descending): equal
        # keys keep (image, in-group rank) ascending, and the live ranks are the first ones.  Negating a float64 is exact.
        order = self._rank((-score, None), (label, C), (image, N))
        at = order.long()
        order2 = self._rank((-score[at], None), (label[at], C))
        scale = None
        if area_scale is not None:
            by_index = sorted(self._index, key=self._index.get)
            scale = torch.from_numpy(np.array([float(area_scale[i]) for i in by_index], np.float64)).to(dev)
        m_bytes, a_bytes = L.y3_coco_match_scratch_bytes(R, self.num_gt), L.y3_coco_ap_scratch_bytes(R)
        scratch = torch.empty(max(m_bytes, a_bytes), dtype=torch.uint8, device=dev)
        words = torch.empty((2, R), dtype=torch.int64, device=dev)
        grank = torch.empty(R, dtype=torch.uint8, device=dev)
        npig = torch.empty((C, 4), dtype=torch.int32, device=dev)
        head, n_prec, n_rec = 12 + 12 * C + 2, 10 * 101 * C * 4 * 3, 10 * C * 4 * 3
        out = torch.zeros(head + n_prec + n_rec, dtype=torch.float64, device=dev)
        stats, per_class, precision, recall = out[:12], out[12:12 + 12 * C], out[head:head + n_prec], out[head + n_prec:]
        iou_thrs = (ctypes.c_double * 10)(*COCO_IOU_THRS)
        rec_thrs = (ctypes.c_double * 101)(*COCO_REC_THRS)
        _lib.check(L.y3_coco_match(ctx, fw.ptr(box), fw.ptr(label), fw.ptr(image), fw.ptr(order), R, fw.ptr(self._state),
                                   fw.ptr(self._gt_start), fw.ptr(self._gt_box), fw.ptr(self._gt_label),
                                   fw.ptr(scale) if scale is not None else None, N, self.num_gt, C, iou_thrs, fw.ptr(scratch),
                                   ctypes.c_size_t(m_bytes), fw.ptr(words[0]), fw.ptr(words[1]), fw.ptr(grank), fw.ptr(npig)))
        _lib.check(L.y3_coco_ap(ctx, fw.ptr(words[0]), fw.ptr(words[1]), fw.ptr(grank), fw.ptr(label), fw.ptr(order), fw.ptr(order2),
                                R, fw.ptr(self._state), fw.ptr(npig), C, rec_thrs, fw.ptr(scratch), ctypes.c_size_t(a_bytes),
                                fw.ptr(precision), fw.ptr(recall)))
        _lib.check(L.y3_coco_summary(ctx, fw.ptr(precision), fw.ptr(recall), C, fw.ptr(per_class), fw.ptr(stats)))
        host = self._read_back(out, head - 2, out.numel() if return_curves else head)
        result = {'stats': host[:12].copy(), 'per_class': host[12:12 + 12 * C].reshape(C, 12).copy()}
        if return_curves:
            result['precision'] = host[head:head + n_prec].reshape(10, 101, C, 4, 3).copy()
            result['recall'] = host[head + n_prec:].reshape(10, C, 4, 3).copy()
        return result
