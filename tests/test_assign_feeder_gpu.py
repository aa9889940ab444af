"""Feeder(assign_iou_thresh=0.213) on the image set tests/test_feeder_gpu.py writes: each batch's y_true is
process_box_batch(batch.boxes, ..., 0.213) - and the host rule - on the boxes the batch carries, and the images are byte for byte
those of the default feeder (the option touches the target assignment only)."""
import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
import assign_cases as AC
import test_feeder_gpu as TF

pytestmark = pytest.mark.gpu


def test_feeder_with_extra_positives(tmp_path):
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.data_utils import process_box_batch
    lines = TF._write_set(tmp_path, 13)
    kw = dict(mode='train', multi_scale=True, use_mix_up=True, num_threads=4, prefetch=2, seed=1)
    plain = Feeder(lines, 8, 80, [416, 416], COCO_ANCHORS, **kw)
    multi = Feeder(lines, 8, 80, [416, 416], COCO_ANCHORS, assign_iou_thresh=AC.DARKNET_THRESH, **kw)
    seen, more = 0, 0
    for a, b in zip(plain.epoch(0), multi.epoch(0)):
        assert a.img_size == b.img_size and torch.equal(a.images, b.images)
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts)
        w, h = b.img_size
        want = process_box_batch(b.boxes, b.labels, b.counts, [w, h], 80, COCO_ANCHORS, AC.DARKNET_THRESH)
        bx, lb, ct = b.boxes.cpu().numpy(), b.labels.cpu().numpy(), b.counts.cpu().numpy()
        rule = AC.host_batch(bx, lb, ct, [w, h], 80, AC.DARKNET_THRESH)
        for got, dev, host, base in zip(b.y_true, want, rule, a.y_true):
            assert torch.equal(got, dev)
            np.testing.assert_array_equal(got.cpu().numpy(), host)
            more += int(got[..., 4].sum()) - int(base[..., 4].sum())
        # the default feeder's targets are the plain call's
        for got, dev in zip(a.y_true, process_box_batch(a.boxes, a.labels, a.counts, [w, h], 80, COCO_ANCHORS)):
            assert torch.equal(got, dev)
        seen += len(b.image_ids)
    assert seen == 13 and more > 0
    plain.close()
    multi.close()
