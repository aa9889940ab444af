# coding: utf-8
"""utils.data_utils of the reference (ref: utils/data_utils.py:17-235) = this package's module under that name: parse_line,
process_box, the resize functions and `get_batch_data` in both modes ('train': mix-up pairing, colour distortion, expand,
constrained crop, random-interpolation resize, flip, multi-scale size every 10 batches; 'val': plain resize), which the
scripts map over their tf.data pipelines (ref: train.py:37-52, eval.py:75-92).  Target assignment runs on the device
(y3_process_box); a dry run (no device) substitutes all-zero targets of the right shape."""
import numpy as np

from yolov3_tensorflow_amd.utils import data_utils as _native
from yolov3_tensorflow_amd.utils.data_utils import *          # noqa: F401,F403
from yolov3_tensorflow_amd.utils.data_utils import (parse_line, process_box, resize_with_bbox, parse_data,   # noqa: F401
                                                    get_batch_data as _get_batch_data)
from yolov3_tensorflow_amd import compat as _compat


def _dry_targets(boxes, labels, counts, img_size, class_num, anchors, assign_iou_thresh=1.0):
    import torch
    n, (w, h) = len(counts), [int(v) for v in img_size]
    return tuple(torch.zeros((n, h // s, w // s, 3, 6 + int(class_num)), dtype=torch.float32) for s in (32, 16, 8))


def get_batch_data(batch_line, class_num, img_size, anchors, mode, multi_scale=False, mix_up=False,
                   letterbox_resize=True, interval=10):
    """A batch of annotation lines -> (image ids int64 [B], images [B,h,w,3], y_true_13, y_true_26, y_true_52)."""
    img_size = [int(v) for v in img_size]
    anchors = np.asarray(anchors, np.float32)
    if not _compat.dry_run():
        return _get_batch_data(batch_line, int(class_num), img_size, anchors, mode, bool(multi_scale), bool(mix_up),
                               bool(letterbox_resize), int(interval))
    real, _native.process_box_batch = _native.process_box_batch, _dry_targets
    try:
        return _get_batch_data(batch_line, int(class_num), img_size, anchors, mode, bool(multi_scale), bool(mix_up),
                               bool(letterbox_resize), int(interval))
    finally:
        _native.process_box_batch = real
