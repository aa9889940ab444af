"""The mosaic composition on the device (include/yolo355.h: y3_mosaic) against its numpy oracle utils.data_aug.mosaic4
(which tests/test_mosaic_cpu.py holds to hand-written pins and a brute-force loop): bit-identical images, boxes, labels and
counts over every case of tests/mosaic_cases.py, on outputs poisoned beforehand; the refusals, each before any launch; one
guard-band case; the feeder end to end (both pixel paths, with and without the source cache) against the oracle applied to
the samples parse_sample gives for the same job keys; and two train steps fed by it."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import mosaic_cases as mc
from conftest import COCO_ANCHORS

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (64, 96)]        # (H, W): a quarter of 8 pixels, so borders fall inside 16-byte groups; H != W


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def poisoned_outputs(n, kmax, H, W, dev):
    return [torch.full((n, H, W, 3), float('nan'), dtype=torch.float32, device=dev),
            torch.full((n, 4 * kmax, 5), float('nan'), dtype=torch.float32, device=dev),
            torch.full((n, 4 * kmax), -1, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev)]


def still_poison(outs):
    torch.cuda.synchronize()
    return bool(torch.isnan(outs[0]).all()) and bool(torch.isnan(outs[1]).all()) and bool((outs[2] == -1).all()) and \
        bool((outs[3] == -1).all())


def raw_call(case, outs=None, records=None, scratch_bytes=None):
    """y3_mosaic itself on device copies of a case: (status, outputs, error text)."""
    from yolov3_tensorflow_amd import _lib, framework as fw
    L, dev = _lib.lib(), fw.default_device()
    n4, H, W, _ = case.images.shape
    n, kmax = n4 // 4, case.boxes.shape[1]
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case.images, case.boxes, case.labels.astype(np.int32),
                                                                      case.counts.astype(np.int32))]
    outs = poisoned_outputs(n, kmax, H, W, dev) if outs is None else outs
    recs = np.ascontiguousarray(case.records if records is None else records, np.int32)
    need = L.y3_mosaic_scratch_bytes(n)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    rc = L.y3_mosaic(fw.context(dev), *[P(t) for t in ins], n, kmax, H, W, recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                     case.min_side, case.min_visible, *[P(t) for t in outs], P(scratch),
                     need if scratch_bytes is None else scratch_bytes)
    text = L.y3_last_error().decode() if rc else ''
    torch.cuda.synchronize()
    return rc, outs, text


def oracle(case):
    from yolov3_tensorflow_amd.utils.data_aug import mosaic4
    return mosaic4(case.images, case.boxes, case.labels, case.counts, case.records, case.min_side, case.min_visible)


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_y3_mosaic_equals_mosaic4_bit_for_bit(size):
    cases = mc.all_cases(*size)
    shapes = {(c.images.shape[0] // 4, c.boxes.shape[1]) for c in cases.values()}
    assert {(n, k) for n in (1, 3) for k in (1, 17, 70)} <= shapes
    for name, case in cases.items():
        rc, outs, text = raw_call(case)
        assert rc == 0, (name, text)
        mc.assert_same([t.cpu().numpy() for t in outs], oracle(case), name)


def test_mosaic_batch_wraps_the_call_and_n0_launches_nothing():
    from yolov3_tensorflow_amd import _lib, framework as fw
    from yolov3_tensorflow_amd.utils.data_utils import mosaic_batch
    case = mc.all_cases(64, 96)['thresholds_n3_k70']
    dev = fw.default_device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = mosaic_batch(t(case.images), t(case.boxes), t(case.labels), t(case.counts), case.records, case.min_side, case.min_visible)
    assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.int32, torch.int32]
    mc.assert_same([g.cpu().numpy() for g in got], oracle(case), 'mosaic_batch')
    with pytest.raises(ValueError, match='image 1'):
        bad = case.records.copy()
        bad[1, 0] = 0
        mosaic_batch(t(case.images), t(case.boxes), t(case.labels), t(case.counts), bad)
    # n = 0: status 0 whatever else is passed, nothing written
    outs = poisoned_outputs(1, 70, 64, 96, dev)
    rec = np.zeros(10, np.int32)
    rc = _lib.lib().y3_mosaic(fw.context(dev), None, None, None, None, 0, 70, 64, 96, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              2.0, 0.25, *[P(o) for o in outs], None, 0)
    assert rc == 0 and still_poison(outs)


def test_refusals_name_the_image_and_launch_nothing():
    from yolov3_tensorflow_amd import _lib
    H, W = 64, 96
    case = mc.random_case(H, W, 3, 17, seed=5, exact=True)
    good = mc.record_with(W, H, 40, 30, 'max')

    def with_record(image, at, value):
        recs = np.asarray([good] * 3, np.int32)
        recs[image, at] = value
        return recs
    refusals = [('cx = 0', 1, 0, 0), ('cx = W', 2, 0, W), ('ox0 = W - tw + 1', 0, 2, W - 40 + 1), ('ox3 = W - tw + 1', 2, 8, 40 + 1),
                ('oy2 = H - th + 1', 1, 7, 30 + 1), ('a negative offset', 2, 4, -1), ('a negative oy', 1, 9, -5)]
    for what, image, at, value in refusals:
        rc, outs, text = raw_call(case, records=with_record(image, at, value))
        assert rc == _lib.Y3_EINVAL and 'image %d' % image in text, (what, rc, text)
        assert still_poison(outs), what
    rc, outs, text = raw_call(case, records=np.asarray([good] * 3, np.int32),
                              scratch_bytes=_lib.lib().y3_mosaic_scratch_bytes(3) - 1)
    assert rc == _lib.Y3_EINVAL and 'scratch' in text and still_poison(outs)
    # ... and the same call with nothing wrong runs
    rc, outs, _ = raw_call(case, records=np.asarray([good] * 3, np.int32))
    assert rc == 0 and not still_poison(outs)


def test_guard_bands_two_images_64x96_kmax17():
    """The entry mosaic_cases.py adds to test_guard_bands_gpu.py's table, through that module's own test: images at exactly
    16-byte alignment, boxes / labels / counts at exactly 4, two poison passes on guards, outputs and scratch; no guard byte
    changed, the passes bit-identical, the oracle's result.  Then the same bytes from the call on plain allocations."""
    import test_guard_bands_gpu as TG
    from yolov3_tensorflow_amd import framework as fw
    mine = [e for e in TG.TABLE if 'y3_mosaic' in e.covers]
    assert len(mine) == 1 and 'y3_mosaic' not in TG.EXCLUDED
    TG.test_guard_bands(mine[0])
    run = mine[0].build(TG.G())
    by_name = {s.name: s for s in run.specs}
    assert by_name['in_images'].align == by_name['out_images'].align == 16
    assert all(by_name[k].align == 4 for k in ('in_boxes', 'in_labels', 'in_counts', 'out_boxes', 'out_labels', 'out_counts'))
    arena = guarded.build(fw.default_device(), run.specs)
    kept = guarded.run_passes(arena, lambda: run.call(arena), run.outputs, sync=torch.cuda.synchronize)
    rc, plain, _ = raw_call(mc.guard_case())
    assert rc == 0
    for name, t in zip(run.outputs, plain):
        assert guarded.bit_identical(kept[0][name], t.cpu()) and guarded.bit_identical(kept[1][name], t.cpu()), name


# -------------------------------------------------------------------------------------------------------------------- the feeder
def _write_set(tmp_path, n, classes=80, seed=5):
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        w, h = int(rng.randint(280, 360)), int(rng.randint(200, 280))
        path = str(tmp_path / ('img_%d.jpg' % i))
        base = rng.randint(0, 256, (h // 8, w // 8, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]).save(path, quality=85)
        parts = ['%d' % i, path, '%d' % w, '%d' % h]
        for _ in range(int(rng.randint(1, 5))):
            x0, y0 = rng.uniform(0, w * 0.5), rng.uniform(0, h * 0.5)
            parts += ['%d' % rng.randint(0, classes), '%.1f' % x0, '%.1f' % y0, '%.1f' % (x0 + rng.uniform(20, w * 0.45)),
                      '%.1f' % (y0 + rng.uniform(20, h * 0.45))]
        lines.append(' '.join(parts))
    return lines


def test_feeder_with_mosaic_equals_the_oracle_on_every_delivery(tmp_path):
    from yolov3_tensorflow_amd.feeder import Feeder, _worker_sample
    from yolov3_tensorflow_amd.utils.data_aug import mosaic4
    from yolov3_tensorflow_amd.utils.data_utils import collate, process_box_batch
    lines = _write_set(tmp_path, 6)
    mk = lambda **kw: Feeder(lines, 2, 80, [416, 416], COCO_ANCHORS, mode='train', multi_scale=True, use_mix_up=True, interval=1,
                             num_threads=4, prefetch=2, seed=4, mosaic=True, **kw)

    def epoch_of(f, epoch=0):
        out = []
        for b in f.epoch(epoch):
            torch.cuda.synchronize()
            out.append((b.image_ids, list(b.img_size), b.images.cpu(), b.boxes.cpu(), b.labels.cpu(), b.counts.cpu(),
                        [y.cpu() for y in b.y_true]))
        f.close()
        return out

    # the oracle: the plan's jobs through the worker function, collated, composed by mosaic4, targets from its boxes
    ref = mk(pixels='host')
    plan = ref._plan(0)
    want = []
    for entry in plan:
        samples = [_worker_sample(job) for job in ref._jobs(0, entry)]
        ids, images, boxes, labels, counts = collate(samples)
        composed = mosaic4(images, boxes, labels, counts, entry[3], ref.mosaic_min_side, ref.mosaic_min_visible)
        y_true = process_box_batch(composed[1], composed[2], composed[3], entry[1], 80, COCO_ANCHORS)
        want.append(([ids[4 * j + own] for j, own in enumerate(entry[4])], list(entry[1]), composed, [y.cpu() for y in y_true]))
    assert len(want) == 3 and len({tuple(w[1]) for w in want}) > 1                 # multi-scale: more than one size
    assert any(isinstance(g, list) for e in plan for group in e[2] for g in group)  # a mix-up pair inside a group
    assert sum(int(w[2][3].sum()) for w in want) > 0

    host = epoch_of(mk(pixels='host'))
    for name, got in (('host', host), ('gpu', epoch_of(mk(pixels='gpu'))), ('gpu, cached', epoch_of(mk(pixels='gpu', cache_bytes=64 << 20)))):
        assert len(got) == len(want), name
        for (ids, size, images, boxes, labels, counts, y_true), (w_ids, w_size, composed, w_y), h in zip(got, want, host):
            assert ids == w_ids and size == w_size and tuple(images.shape) == (len(ids), size[1], size[0], 3), name
            mc.assert_same([images.numpy(), boxes.numpy(), labels.numpy(), counts.numpy()], composed, name)
            assert all(torch.equal(a, b) for a, b in zip(y_true, w_y)), name
            assert torch.equal(images, h[2]) and torch.equal(boxes, h[3])           # byte-equal batches on every delivery

    # switched off between epochs: the batches of a feeder that never had it
    f = mk(pixels='gpu')
    f.mosaic = False
    plain = Feeder(lines, 2, 80, [416, 416], COCO_ANCHORS, mode='train', multi_scale=True, use_mix_up=True, interval=1,
                   num_threads=4, prefetch=2, seed=4, pixels='gpu')
    for a, b in zip(epoch_of(f, 1), epoch_of(plain, 1)):
        assert a[0] == b[0] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and all(torch.equal(x, y) for x, y in zip(a[6], b[6]))


def test_two_train_steps_fed_by_the_mosaic_feeder(tmp_path, isolated_graph):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    lines = _write_set(tmp_path, 4, seed=8)
    y3.reset_default_graph()
    model = y3.yolov3(80, COCO_ANCHORS, batch_norm_decay=0.99)
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
        trainer = training.Trainer(model, config_optimizer('momentum', 1e-3))
        feeder = Feeder(lines, 2, 80, [96, 64], COCO_ANCHORS, mode='train', use_mix_up=True, num_threads=2, prefetch=2, seed=3,
                        mosaic=True)
        watched = [v for v in y3.global_variables(scope='yolov3') if v.op_name.endswith('/weights')]
        before = [v.tensor.clone() for v in (watched[0], watched[-1])]
        losses = []
        for batch in feeder.epoch(0):
            assert tuple(batch.images.shape) == (2, 64, 96, 3) and batch.boxes.shape[1] % 4 == 0
            losses.append([float(v) for v in trainer.step(batch.images, batch.y_true)])
        feeder.close()
    assert len(losses) == 2 and np.isfinite(np.asarray(losses)).all(), losses
    for v, b in zip((watched[0], watched[-1]), before):
        assert torch.isfinite(v.tensor).all() and not torch.equal(v.tensor, b), v.name
