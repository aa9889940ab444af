"""The affine warp on the device (include/yolo355.h: y3_affine) against its numpy oracle utils.data_aug.affine_warp (which
tests/test_affine_cpu.py holds to hand-written pins and a brute-force loop): bit-identical images, boxes, labels and counts
over every case of tests/affine_cases.py and at sizes that are no multiple of the pixel kernel's 32 x 32 tile, on outputs
poisoned beforehand; the refusals, each before any launch; one guard-band case; the feeder end to end on every delivery, with
and without mosaic, against the oracle applied to the same feeder's batches without the warp."""
import ctypes
import random

import numpy as np
import pytest
import torch

import guarded
import affine_cases as ac
from conftest import COCO_ANCHORS

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (64, 96)]        # (H, W)
ODD_SIZES = [(5, 7), (37, 45), (33, 130)]       # below one tile; tiles cut on both sides; five tiles across, two bands down


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def poisoned_outputs(n, kmax, H, W, dev):
    return [torch.full((n, H, W, 3), float('nan'), dtype=torch.float32, device=dev),
            torch.full((n, kmax, 5), float('nan'), dtype=torch.float32, device=dev),
            torch.full((n, kmax), -1, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev)]


def still_poison(outs):
    torch.cuda.synchronize()
    return bool(torch.isnan(outs[0]).all()) and bool(torch.isnan(outs[1]).all()) and bool((outs[2] == -1).all()) and \
        bool((outs[3] == -1).all())


def as_words(records):
    return np.ascontiguousarray((np.asarray(records, np.int64) & 0xffffffff).astype(np.uint32).view(np.int32))


def raw_call(case, records=None, scratch_bytes=None, size=None):
    """y3_affine itself on device copies of a case: (status, outputs, error text).  size: the (H, W) to pass, where it is not
    the tensors' own."""
    from yolov3_tensorflow_amd import _lib, framework as fw
    L, dev = _lib.lib(), fw.default_device()
    n, H, W, _ = case.images.shape
    kmax = case.boxes.shape[1]
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case.images, case.boxes, case.labels.astype(np.int32),
                                                                      case.counts.astype(np.int32))]
    outs = poisoned_outputs(n, kmax, H, W, dev)
    recs = as_words(case.records if records is None else records)
    need = L.y3_affine_scratch_bytes(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    H, W = (H, W) if size is None else size
    rc = L.y3_affine(fw.context(dev), *[P(t) for t in ins], n, kmax, H, W, recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                     case.fill, case.min_side, case.min_area, case.max_aspect, *[P(t) for t in outs], P(scratch),
                     need if scratch_bytes is None else scratch_bytes)
    text = L.y3_last_error().decode() if rc else ''
    torch.cuda.synchronize()
    return rc, outs, text


def oracle(case):
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp
    return affine_warp(case.images, case.boxes, case.labels, case.counts, case.records, case.fill, case.min_side,
                       case.min_area, case.max_aspect)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_y3_affine_equals_affine_warp_bit_for_bit(size):
    cases = ac.all_cases(*size)
    shapes = {(c.images.shape[0], c.boxes.shape[1]) for c in cases.values()}
    assert {(n, k) for n in (1, 3) for k in ac.KMAXES} <= shapes
    for name, case in cases.items():
        rc, outs, text = raw_call(case)
        assert rc == 0, (name, text)
        ac.assert_same([t.cpu().numpy() for t in outs], oracle(case), name)


@pytest.mark.parametrize('size', ODD_SIZES, ids=lambda s: '%dx%d' % s)
def test_y3_affine_at_sizes_that_are_no_multiple_of_the_tile(size):
    H, W = size
    prng = random.Random(H * W)
    records = [ac.IDENTITY, ac.shift(-0.5, -0.5), ac.drawn(prng, W, H, ac.MODEST), ac.drawn(prng, W, H, ac.WIDEST)]
    case = ac.case_of(ac.noise_pixels(4, H, W, H + W), records, 9, seed=H)
    rc, outs, text = raw_call(case)
    assert rc == 0, text
    want = oracle(case)
    assert want[0][0].tobytes() == case.images[0].tobytes()
    ac.assert_same([t.cpu().numpy() for t in outs], want, 'odd')


def test_affine_batch_wraps_the_call_and_n0_launches_nothing():
    from yolov3_tensorflow_amd import _lib, framework as fw
    from yolov3_tensorflow_amd.utils.data_utils import affine_batch, pad_fill
    case = ac.all_cases(64, 96)['thresholds_n3_k70']
    dev = fw.default_device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = affine_batch(t(case.images), t(case.boxes), t(case.labels), t(case.counts), case.records, case.fill, case.min_side,
                       case.min_area, case.max_aspect)
    assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.int32, torch.int32]
    ac.assert_same([g.cpu().numpy() for g in got], oracle(case), 'affine_batch')
    # the default fill is the letterbox padding's grey
    moved = [ac.shift(7, 5)] * 3
    got = affine_batch(t(case.images), t(case.boxes), t(case.labels), t(case.counts), moved)
    assert (got[0][:, :5, :, :].cpu() == np.float32(pad_fill())).all() and ac.FILL == pad_fill()
    with pytest.raises(ValueError, match='image 1: word 3, id='):
        bad = case.records.copy()
        bad[1, 3] = -(1 << 20) - 1
        affine_batch(t(case.images), t(case.boxes), t(case.labels), t(case.counts), bad)
    # n = 0: status 0 whatever else is passed, nothing written
    outs = poisoned_outputs(1, 70, 64, 96, dev)
    rec = np.zeros(12, np.int32)
    rc = _lib.lib().y3_affine(fw.context(dev), None, None, None, None, 0, 70, 64, 96, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              0.5, 2.0, 0.1, 20.0, *[P(o) for o in outs], None, 0)
    assert rc == 0 and still_poison(outs)


def test_refusals_name_the_image_and_the_word_and_launch_nothing():
    from yolov3_tensorflow_amd import _lib
    H, W = 64, 96
    case = ac.case_of(ac.noise_pixels(3, H, W, 5), [ac.shift(1.5, 2)] * 3, 17, seed=5)

    def with_word(image, word, value):
        recs = np.asarray(case.records, np.int64).copy()
        recs[image, word] = value
        return recs
    refusals = [('ia above', 1, 0, (1 << 20) + 1, 'ia'), ('ib below', 2, 1, -(1 << 20) - 1, 'ib'), ('ic above', 0, 2, (1 << 30) + 1, 'ic'),
                ('id above', 2, 3, 1 << 21, 'id'), ('ie below', 1, 4, -(1 << 31), 'ie'), ('if below', 2, 5, -(1 << 30) - 1, 'if'),
                ('fa infinite', 0, 6, ac.bits(float('inf')), 'fa'), ('fc NaN', 1, 8, ac.bits(float('nan')), 'fc'),
                ('ff -infinite', 2, 11, ac.bits(float('-inf')), 'ff')]
    for what, image, word, value, name in refusals:
        rc, outs, text = raw_call(case, records=with_word(image, word, value))
        assert rc == _lib.Y3_EINVAL and 'image %d' % image in text and 'word %d, %s' % (word, name) in text, (what, rc, text)
        if word < 6:
            bound = 1 << 30 if word in (2, 5) else 1 << 20
            assert '%s=%d outside [%d, %d]' % (name, value, -bound, bound) in text, text
        assert still_poison(outs), what
    rc, outs, text = raw_call(case, scratch_bytes=_lib.lib().y3_affine_scratch_bytes(3) - 1)
    assert rc == _lib.Y3_EINVAL and 'scratch' in text and still_poison(outs)
    # a side beyond 4096 (the tensors are as large as the call says: a missing refusal would stay inside them)
    for size in ((1, 4097), (4097, 1)):
        wide = ac.case_of(np.zeros((1,) + size + (3,), np.float32), [ac.IDENTITY], 1, seed=1)
        rc, outs, text = raw_call(wide)
        assert rc == _lib.Y3_EINVAL and '4096' in text and still_poison(outs), (size, text)
    rc, outs, text = raw_call(case, size=(0, 96))
    assert rc == _lib.Y3_EINVAL and still_poison(outs)
    nan_rule = case._replace(min_area=float('nan'))
    rc, outs, text = raw_call(nan_rule)
    assert rc == _lib.Y3_EINVAL and 'NaN' in text and still_poison(outs)
    # ... and the same call with nothing wrong runs
    rc, outs, _ = raw_call(case)
    assert rc == 0 and not still_poison(outs)


def test_guard_bands_two_images_64x96_kmax17():
    """The entry affine_cases.py adds to test_guard_bands_gpu.py's table, through that module's own test: every tensor at
    exactly 4-byte alignment, two poison passes on guards, outputs and scratch; no guard byte changed, the passes
    bit-identical, the oracle's result.  Then the same bytes from the call on plain allocations."""
    import test_guard_bands_gpu as TG
    from yolov3_tensorflow_amd import framework as fw
    mine = [e for e in TG.TABLE if 'y3_affine' in e.covers]
    assert len(mine) == 1 and 'y3_affine' not in TG.EXCLUDED
    TG.test_guard_bands(mine[0])
    run = mine[0].build(TG.G())
    by_name = {s.name: s for s in run.specs}
    assert all(by_name[k].align == 4 for k in ('in_images', 'in_boxes', 'in_labels', 'in_counts', 'out_images', 'out_boxes',
                                               'out_labels', 'out_counts'))
    arena = guarded.build(fw.default_device(), run.specs)
    kept = guarded.run_passes(arena, lambda: run.call(arena), run.outputs, sync=torch.cuda.synchronize)
    rc, plain, _ = raw_call(ac.guard_case())
    assert rc == 0
    for name, t in zip(run.outputs, plain):
        assert guarded.bit_identical(kept[0][name], t.cpu()) and guarded.bit_identical(kept[1][name], t.cpu()), name


# -------------------------------------------------------------------------------------------------------------------- the feeder
DELIVERIES = [dict(backend='thread', pixels='host'), dict(backend='thread', pixels='gpu'),
              dict(backend='thread', pixels='gpu', cache_bytes=64 << 20), dict(backend='process')]


def epoch_of(f, epoch=0):
    """One epoch's batches, every tensor read on the default stream right after the yield, with no synchronisation in
    between: the consumer's ordering behind the side stream is the feeder's business."""
    out = []
    for b in f.epoch(epoch):
        out.append((b.image_ids, list(b.img_size), b.images.cpu(), b.boxes.cpu(), b.labels.cpu(), b.counts.cpu(),
                    [y.cpu() for y in b.y_true]))
    f.close()
    return out


@pytest.mark.parametrize('mosaic', [False, True], ids=['plain', 'mosaic'])
def test_feeder_with_affine_equals_the_oracle_on_every_delivery(tmp_path, mosaic):
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp
    from yolov3_tensorflow_amd.utils.data_utils import pad_fill, process_box_batch
    lines = ac.feeder_set(tmp_path, 8)
    for delivery in DELIVERIES:
        mk = lambda **kw: Feeder(lines, 4, 80, [96, 64], COCO_ANCHORS, mode='train', use_mix_up=True, num_threads=2, prefetch=2,
                                 seed=4, mosaic=mosaic, **dict(delivery, **kw))
        name = '%r mosaic=%d' % (sorted(delivery.items()), mosaic)
        plain = epoch_of(mk())
        assert len(plain) == 2 and all(tuple(b[2].shape) == (4, 64, 96, 3) for b in plain) and sum(int(b[5].sum()) for b in plain) > 0
        # the warp: the oracle applied to the batches of the same feeder without it, with the feeder's own records
        f = mk(affine=ac.WIDEST)
        records = [f._affine_records(0, entry, f.affine) for entry in f._plan(0)]
        got = epoch_of(f)
        assert len(got) == 2
        changed = 0
        for (ids, size, images, boxes, labels, counts, y_true), before, recs in zip(got, plain, records):
            want = affine_warp(before[2].numpy(), before[3].numpy(), before[4].numpy(), before[5].numpy(), recs, pad_fill(),
                               f.affine_min_side, f.affine_min_area, f.affine_max_aspect)
            assert ids == before[0] and size == before[1] == [96, 64], name
            ac.assert_same([images.numpy(), boxes.numpy(), labels.numpy(), counts.numpy()], want, name)
            want_y = process_box_batch(want[1], want[2], want[3], size, 80, COCO_ANCHORS)
            assert all(torch.equal(a, b.cpu()) for a, b in zip(y_true, want_y)), name
            changed += int(not torch.equal(images, before[2]))
        assert changed == 2, name
        # every range zero: the batches of the feeder without the warp (no box of this set is near a rule of the filter)
        for a, b in zip(epoch_of(mk(affine=(0.0, 0.0, 0.0, 0.0))), plain):
            assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[2:6], b[2:6])), name
            assert all(torch.equal(x, y) for x, y in zip(a[6], b[6])), name
        # switched off between epochs: the batches of a feeder that never had it
        f = mk(affine=ac.MODEST)
        f.affine = None
        for a, b in zip(epoch_of(f, 1), epoch_of(mk(), 1)):
            assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[2:6], b[2:6])), name
