"""y3_process_box_multi (multi-anchor positives in the target assignment, include/yolo355.h) through the C ABI against the
host form of the rule, utils.data_utils.process_box_host, bit for bit: a 96 x 64 image (grids 3 x 2, 6 x 4, 12 x 8: an exchange
of w and h shows), counts (6, 0, 3), the hand cases of tests/assign_cases.py, an out-of-range label, a centre outside the image,
a pair of boxes that collide on a record; the option off (thresholds 1 and 2) against y3_process_box; refusals; guard bands."""
import numpy as np
import pytest

from conftest import COCO_ANCHORS
import assign_cases as AC

pytestmark = pytest.mark.gpu

SIZE = [AC.GPU_W, AC.GPU_H]


@pytest.mark.parametrize('thresh', [0.213, 0.5])
def test_multi_anchor_assignment_is_the_host_rule_bit_for_bit(thresh):
    boxes, labels, counts = AC.gpu_case()
    want = AC.host_batch(boxes, labels, counts, SIZE, AC.GPU_C, thresh)
    rc, got = AC.device_assign(boxes, labels, counts, SIZE, AC.GPU_C, thresh, poison=float('nan'))
    assert rc == 0
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
    # the option does something here: more object records than the best anchors alone give
    plain = AC.host_batch(boxes, labels, counts, SIZE, AC.GPU_C, 1.0)
    assert sum(int(y[..., 4].sum()) for y in want) > sum(int(y[..., 4].sum()) for y in plain)
    # again: the same bytes
    rc, again = AC.device_assign(boxes, labels, counts, SIZE, AC.GPU_C, thresh, poison=3.0e38)
    assert rc == 0 and all(np.array_equal(a.view(np.uint32), g.view(np.uint32)) for a, g in zip(again, got))


def _coco_square_case():
    rng = np.random.RandomState(4)
    n, kmax, W = 2, 9, 416
    boxes, labels, counts = np.zeros((n, kmax, 5), np.float32), np.zeros((n, kmax), np.int32), np.array([9, 5], np.int32)
    for i, K in enumerate(counts):
        wh, c = rng.uniform(6, 300, (K, 2)), rng.uniform(1, W - 1, (K, 2))
        boxes[i, :K] = np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(0.05, 0.95, (K, 1))], 1)
        labels[i, :K] = rng.randint(0, 80, K)
    return boxes, labels, counts


@pytest.mark.parametrize('thresh', [1.0, 2.0])
def test_with_the_option_off_it_is_y3_process_box_bit_for_bit(thresh):
    for (boxes, labels, counts), size, C in ((AC.gpu_case(), SIZE, AC.GPU_C), (_coco_square_case(), [416, 416], 80)):
        rc0, plain = AC.device_assign(boxes, labels, counts, size, C, None, poison=float('nan'), entry='y3_process_box')
        rc1, multi = AC.device_assign(boxes, labels, counts, size, C, thresh, poison=float('nan'))
        assert rc0 == 0 and rc1 == 0
        for p, m in zip(plain, multi):
            assert np.array_equal(p.view(np.uint32), m.view(np.uint32))
        for p, w in zip(plain, AC.host_batch(boxes, labels, counts, size, C, 1.0)):
            np.testing.assert_array_equal(p, w)


def test_python_process_box_takes_the_threshold():
    from yolov3_tensorflow_amd.utils import data_utils
    boxes, labels, counts = AC.gpu_case()
    ys = data_utils.process_box_batch(boxes, labels, counts, SIZE, AC.GPU_C, COCO_ANCHORS, 0.213)
    for y, w in zip(ys, AC.host_batch(boxes, labels, counts, SIZE, AC.GPU_C, 0.213)):
        np.testing.assert_array_equal(y.cpu().numpy(), w)
    one = data_utils.process_box(boxes[0], labels[0], SIZE, AC.GPU_C, COCO_ANCHORS, assign_iou_thresh=0.213)
    for y, w in zip(one, AC.host(boxes[0], labels[0], SIZE, AC.GPU_C, 0.213)):
        np.testing.assert_array_equal(y, w)
    for y, w in zip(data_utils.process_box(boxes[0], labels[0], SIZE, AC.GPU_C, COCO_ANCHORS), AC.host(boxes[0], labels[0], SIZE, AC.GPU_C, 1.0)):
        np.testing.assert_array_equal(y, w)


@pytest.mark.parametrize('thresh', [0.0, -1.0, float('nan')])
def test_bad_thresholds_are_refused_and_the_outputs_untouched(thresh):
    from yolov3_tensorflow_amd import _lib
    boxes, labels, counts = AC.gpu_case()
    rc, got = AC.device_assign(boxes, labels, counts, SIZE, AC.GPU_C, thresh, poison=-7.25)
    assert rc == _lib.Y3_EINVAL
    assert all((g == -7.25).all() for g in got)


def test_guard_bands_of_the_96x64_call():
    """the entry assign_cases.py adds to test_guard_bands_gpu.py's table, through that module's own test (docs/guard_bands.md):
    two passes on poisoned guards and outputs; no guard byte changed, the passes bit-identical, the host rule bit for bit"""
    import test_guard_bands_gpu as TG
    mine = [e for e in TG.TABLE if 'y3_process_box_multi' in e.covers]
    assert len(mine) == 1
    TG.test_guard_bands(mine[0])
