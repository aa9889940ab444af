"""The feeder's pixel work on the device (y3_feed_run, include/yolo355.h; reference
utils/data_utils.py:118-172 after its draws): the three kernels against liby3feed.so's y3f_sample - which is itself
held bit for bit to the numpy / Pillow definition (tests/test_feed_native.py) - on the random jobs of feed_cases.py, on
full-size jobs, and through the Feeder."""
import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
from feed_cases import describe, random_case, random_image

pytestmark = pytest.mark.gpu


def _compare(cases, fn, got):
    got = got.cpu().numpy()
    bad = []
    for i, c in enumerate(cases):
        want = fn.sample(as_float=True, **c)
        if not np.array_equal(got[i], want):
            y, x, ch = np.argwhere(got[i] != want)[0]
            bad.append('%s\n   first difference at (y %d, x %d, c %d): %r != %r (%d pixels differ)' %
                       (describe(c), y, x, ch, got[i][y, x, ch] * 255, want[y, x, ch] * 255, int((got[i] != want).any(-1).sum())))
    assert not bad, '%d of %d cases differ:\n%s' % (len(bad), len(cases), '\n'.join(bad[:5]))


@pytest.mark.parametrize('interp', range(5))
def test_kernels_equal_y3f_sample_on_random_jobs(interp):
    from yolov3_tensorflow_amd import feed_native as fn
    from yolov3_tensorflow_amd.feed_device import DevicePixels
    rng = np.random.RandomState(200 + interp)
    dp = DevicePixels()
    for size in ((32, 32), (48, 48), (64, 64)):
        cases = [random_case(rng, out_size=size, interp=interp) for _ in range(150)]
        _compare(cases, fn, dp.run([fn.make_job(**c) for c in cases]))


def test_kernels_equal_y3f_sample_at_training_size():
    """640x480 sources, mix-up partners of another size, 4x expansion, every interpolation, letterbox to 416 and plain
    resize to 608: long filter windows (LANCZOS4 over a 2,500-pixel canvas: 37 taps), large scratch, one batch of 40."""
    from yolov3_tensorflow_amd import feed_native as fn
    from yolov3_tensorflow_amd.feed_device import DevicePixels
    rng = np.random.RandomState(3)
    dp = DevicePixels()
    for out in (416, 608):
        cases = []
        for i in range(40):
            img1 = random_image(rng, 480, 640)
            img2 = random_image(rng, 427, 640) if i % 3 == 0 else None
            mh, mw = 480, 640
            ratio = rng.uniform(1, 4) if i % 2 else 1.0
            cw, ch = int(mw * ratio), int(mh * ratio)
            off = (int(rng.randint(0, cw - mw + 1)), int(rng.randint(0, ch - mh + 1)))
            ww, wh = int(rng.randint(cw // 3, cw + 1)), int(rng.randint(ch // 3, ch + 1))
            window = (int(rng.randint(0, cw - ww + 1)), int(rng.randint(0, ch - wh + 1)), ww, wh)
            if out == 416:
                scale = min(out / ww, out / wh)
                resized = (max(1, int(ww * scale)), max(1, int(wh * scale)))
                pad = ((out - resized[0]) // 2, (out - resized[1]) // 2)
            else:
                resized, pad = (out, out), (0, 0)
            cases.append(dict(img1=img1, img2=img2, lam=float(rng.beta(1.5, 1.5)) if img2 is not None else 1.0,
                              colour=(int(rng.randint(-32, 33)), int(rng.randint(-18, 19)), float(rng.uniform(0.5, 1.5)),
                                      float(rng.uniform(0.5, 1.5))) if i % 4 else None,
                              offset=off, window=window, interp=i % 5, resized=resized, out_size=(out, out), pad=pad,
                              pad_value=128, flip_x=bool(i % 2)))
        _compare(cases, fn, dp.run([fn.make_job(**c) for c in cases], threads=4))


def test_every_colour_goes_through_the_device_jitter_like_the_host():
    """All 2^24 RGB values as one 4096x4096 image through an identity resize, with a jitter and without."""
    from yolov3_tensorflow_amd import feed_native as fn
    from yolov3_tensorflow_amd.feed_device import DevicePixels
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    dp = DevicePixels()
    for colour in ((0, None, None, None), (11, -13, 1.31, 0.77), (-20, 17, 0.6, 1.4)):
        case = dict(img1=img, colour=colour, interp=1, out_size=(4096, 4096))
        got = dp.run([fn.make_job(**case)]).cpu().numpy()[0]
        want = fn.sample(as_float=True, **case)
        assert np.array_equal(got, want), 'jitter %r: %d colours differ' % (colour, int((got != want).any(-1).sum()))


def _packed_plan(runner, rng, accept):
    """Three random 32x32 jobs, all sources packed (no arena), drawn until accept(records, blob) holds."""
    while True:
        cases = [random_case(rng, out_size=(32, 32)) for _ in range(3)]
        p = runner.plan(cases, np.zeros(16, np.uint8), [None] * 3, [None] * 3)
        if accept(p['recs'], p['blob']):
            return cases, p


def test_run_reports_bad_arguments():
    """The one entry on a PACKED plan: what it must refuse before launching anything, each followed by a good call."""
    from feed_src_cases import Runner
    runner = Runner()
    fn, EINVAL = runner.fn, runner._lib.Y3_EINVAL
    rng = np.random.RandomState(0)
    live = lambda d: (d.live_x1 - d.live_x0) * (d.live_y1 - d.live_y0)
    hpass = lambda d: d.mode == 4 and d.horizontal and d.tmp_rows > 0
    cases, p = _packed_plan(runner, rng, lambda recs, blob: all(live(d) and d.r1_w * d.r1_h for d in recs) and any(hpass(d) for d in recs))
    recs, n, blob_bytes = p['recs'], 3, p['blob'].size
    assert all(tuple(d.reserved) == (0, 0, 0) for d in recs)

    def good(**kw):
        p['out'].fill_(float('nan'))
        assert runner.call(p, arena=False, src_bytes=0, **kw) == 0, runner.lib.y3_last_error()
        _compare(cases, fn, p['out'])

    def refused(what, **kw):
        p['out'].fill_(float('nan'))
        assert runner.call(p, arena=False, src_bytes=0, **kw) == EINVAL
        message = runner.lib.y3_last_error()
        assert what in message, message
        torch.cuda.synchronize()
        assert torch.isnan(p['out']).all()          # nothing was launched
        good()

    def edited(change, of=None):
        copy = (fn.DJob * n).from_buffer_copy(bytes(recs if of is None else of))
        change(copy)
        return copy

    good()
    refused(b'the batch is', out_hw=(48, 32))                       # a wrong output size
    # the scratch: what the jobs write, 16-aligned, then the records; that much is enough and 16 bytes less is not
    need = max(max(d.win_off + live(d) * 3, d.tmp_off + (d.tmp_rows * d.res_w * 3 if hpass(d) else 0)) for d in recs)
    enough = (need + 15) // 16 * 16 + n * 208
    assert 16 < enough <= p['scratch'].numel()
    good(scratch_bytes=enough)
    refused(b'scratch', scratch_bytes=enough - 16)
    refused(b'null argument', blob=False)                           # a NULL blob
    # a packed source that ends one byte past blob_bytes
    k = 1
    size = recs[k].r1_w * recs[k].r1_h * 3
    refused(b'job %d: packed source past the blob' % k, recs=edited(lambda r: setattr(r[k], 'img1_off', blob_bytes - size + 1)))
    # a live rectangle wider than the window
    refused(b'job %d: live rectangle outside the window' % k, recs=edited(lambda r: setattr(r[k], 'live_x1', r[k].win_w + 1)))
    # a horizontal pass whose rows run past the scratch
    k = next(i for i, d in enumerate(recs) if hpass(d))
    rows = (p['scratch'].numel() - recs[k].tmp_off) // (recs[k].res_w * 3) + 1
    assert recs[k].tmp_off + rows * recs[k].res_w * 3 > p['scratch'].numel()
    refused(b'job %d: ' % k, recs=edited(lambda r: setattr(r[k], 'tmp_rows', rows)))
    # stale records: those of another batch, whose blob is larger and whose last job's y table is that blob's last piece
    tabled = lambda d: d.mode in (0, 1) or (d.mode == 4 and d.vertical)
    _, other = _packed_plan(runner, rng, lambda r, blob: blob.size > blob_bytes + 16 and tabled(r[2]) and
                            r[2].ytab_off + r[2].res_h * 4 > blob_bytes)
    refused(b': job ', recs=edited(lambda r: None, of=other['recs']))
    # a blob too small to hold the records themselves
    refused(b'records do not fit', blob_bytes=n * 208 - 1)


def test_feeder_with_device_pixels_serves_the_batches_of_the_host_path(tmp_path):
    from test_feeder_gpu import _write_set
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = _write_set(tmp_path, 37)
    kw = dict(mode='train', multi_scale=True, use_mix_up=True, num_threads=6, prefetch=3, seed=4, interval=2)
    host = Feeder(lines, 8, 80, [416, 416], COCO_ANCHORS, pixels='host', **kw)
    gpu = Feeder(lines, 8, 80, [416, 416], COCO_ANCHORS, pixels='gpu', **kw)
    served = 0
    for a, b in zip(host.epoch(0), gpu.epoch(0)):
        assert a.image_ids == b.image_ids and a.img_size == b.img_size
        assert b.images.is_cuda and torch.equal(a.images, b.images)
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts)
        assert all(torch.equal(x, y) for x, y in zip(a.y_true, b.y_true))
        served += len(b.image_ids)
    assert served == 37
    # validation mode: plain letterbox, no draws
    host = Feeder(lines[:9], 4, 80, [416, 416], COCO_ANCHORS, mode='val', num_threads=3, pixels='host')
    gpu = Feeder(lines[:9], 4, 80, [416, 416], COCO_ANCHORS, mode='val', num_threads=3, pixels='gpu')
    for a, b in zip(host.epoch(0), gpu.epoch(0)):
        assert torch.equal(a.images, b.images)
    with pytest.raises(ValueError):
        Feeder(lines, 8, 80, [416, 416], COCO_ANCHORS, backend='process', pixels='gpu')
