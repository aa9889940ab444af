"""The feeder's pixel work over sources kept in HBM (y3f_plan_batch_src + y3_feed_run, include/yolo355.h): the kernels
against liby3feed.so's y3f_sample on mixed batches (sources in an arena next to packed ones), at training geometry, with
bad arguments, and through Feeder(cache_bytes=...), whose batches must be the uncached feeder's byte for byte - also once
the files are gone from the disk."""
import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS
from feed_cases import describe, random_case, random_image
from feed_src_cases import Runner, place, ref_jobs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def runner():
    return Runner()


def _compare(cases, fn, got, src1, src2):
    got = got.cpu().numpy()
    bad = []
    for i, c in enumerate(cases):
        want = fn.sample(as_float=True, **c)
        if not np.array_equal(got[i], want):
            y, x, ch = np.argwhere(got[i] != want)[0]
            bad.append('%s\n   sources at %r / %r, first difference at (y %d, x %d, c %d): %r != %r (%d pixels differ)' %
                       (describe(c), src1[i], src2[i], y, x, ch, got[i][y, x, ch] * 255, want[y, x, ch] * 255,
                        int((got[i] != want).any(-1).sum())))
    assert not bad, '%d of %d cases differ:\n%s' % (len(bad), len(cases), '\n'.join(bad[:5]))


@pytest.mark.parametrize('interp', range(5))
def test_kernels_equal_y3f_sample_on_a_mixed_batch(runner, interp):
    rng = np.random.RandomState(400 + interp)
    cases = [random_case(rng, out_size=(48, 48), interp=interp) for _ in range(64)]
    arena, src1, src2 = place(rng, cases)
    p = runner.plan(cases, arena, src1, src2)
    assert runner.call(p) == 0, runner.lib.y3_last_error()
    _compare(cases, runner.fn, p['out'], src1, src2)
    assert np.array_equal(p['arena'].cpu().numpy(), arena)


def test_kernels_equal_y3f_sample_at_training_size(runner):
    """640x480 sources (rows of 1,920 bytes read in place) with mix-up partners, 4x expansion, letterbox to 416x416, every
    source in the arena: 173,056 output pixels per job are 676 blocks of work for a grid capped at 512."""
    rng = np.random.RandomState(3)
    cases = []
    for i in range(8):
        img1 = random_image(rng, 480, 640)
        img2 = random_image(rng, 427, 640) if i % 2 == 0 else None
        ratio = rng.uniform(2, 4) if i % 4 < 2 else 1.0
        cw, ch = int(640 * ratio), int(480 * ratio)
        off = (int(rng.randint(0, cw - 640 + 1)), int(rng.randint(0, ch - 480 + 1)))
        ww, wh = int(rng.randint(cw // 2, cw + 1)), int(rng.randint(ch // 2, ch + 1))
        window = (int(rng.randint(0, cw - ww + 1)), int(rng.randint(0, ch - wh + 1)), ww, wh)
        scale = min(416 / ww, 416 / wh)
        resized = (max(1, int(ww * scale)), max(1, int(wh * scale)))
        cases.append(dict(img1=img1, img2=img2, lam=float(rng.beta(1.5, 1.5)) if img2 is not None else 1.0,
                          colour=(int(rng.randint(-32, 33)), int(rng.randint(-18, 19)), float(rng.uniform(0.5, 1.5)),
                                  float(rng.uniform(0.5, 1.5))) if i % 3 else None,
                          offset=off, window=window, interp=i % 5, resized=resized, out_size=(416, 416),
                          pad=((416 - resized[0]) // 2, (416 - resized[1]) // 2), pad_value=128, flip_x=bool(i % 2)))
    arena, src1, src2 = place(rng, cases, cache_all=True)
    p = runner.plan(cases, arena, src1, src2)
    assert all(d.reserved[0] == (3 if d.has2 else 1) and d.reserved[1] == 640 for d in p['recs'])
    assert runner.call(p) == 0, runner.lib.y3_last_error()
    _compare(cases, runner.fn, p['out'], src1, src2)


def test_bad_arguments_are_refused_and_nothing_runs(runner):
    rng = np.random.RandomState(12)
    cases = [random_case(rng, out_size=(32, 32)) for _ in range(12)]
    arena, src1, src2 = place(rng, cases, cache_all=True)
    p = runner.plan(cases, arena, src1, src2)
    fn, EINVAL = runner.fn, runner._lib.Y3_EINVAL
    n = p['n']

    def edited(change):
        recs = (fn.DJob * n).from_buffer_copy(bytes(p['recs']))
        change(recs)
        return recs

    def good():
        p['out'].fill_(float('nan'))
        assert runner.call(p) == 0, runner.lib.y3_last_error()
        _compare(cases, fn, p['out'], src1, src2)

    def refused(what, **kw):
        p['out'].fill_(float('nan'))
        assert runner.call(p, **kw) == EINVAL
        message = runner.lib.y3_last_error()
        assert what in message, message
        with pytest.raises(ValueError):
            runner._lib.check(EINVAL)
        torch.cuda.synchronize()
        assert torch.isnan(p['out']).all()          # nothing was launched
        good()

    good()
    # an arena rectangle one byte past src_bytes: the arena cut just short of the farthest rectangle's last byte
    ends = [getattr(d, 'img%d_off' % s) + ((getattr(d, 'r%d_y0' % s) + getattr(d, 'r%d_h' % s) - 1) * d.reserved[s] +
                                           getattr(d, 'r%d_x0' % s) + getattr(d, 'r%d_w' % s)) * 3
            for d in p['recs'] for s in ((1, 2) if d.has2 else (1,)) if getattr(d, 'r%d_w' % s) * getattr(d, 'r%d_h' % s)]
    far = max(ends)
    assert runner.call(p, src_bytes=far) == 0
    refused(b'past the arena', src_bytes=far - 1)
    # a table offset past blob_bytes
    k = next(i for i, d in enumerate(p['recs']) if d.mode in (0, 1) or (d.mode == 4 and d.vertical))
    refused(b'job %d: table past the blob' % k, recs=edited(lambda r: setattr(r[k], 'ytab_off', p['blob'].size)))
    # src_dev NULL with a referring record
    refused(b'past the arena', arena=False)
    # a stride smaller than r_x0 + r_w
    k = next(i for i, d in enumerate(p['recs']) if d.r1_w * d.r1_h)
    narrow = p['recs'][k].r1_x0 + p['recs'][k].r1_w - 1
    refused(b'job %d: arena row stride' % k, recs=edited(lambda r: r[k].reserved.__setitem__(1, narrow)))
    # and what the records' own blob must hold: a blob size that cuts a job's last table
    refused(b'blob', blob_bytes=p['blob'].size - 16)


def _write_small_set(folder, n, seed=9):
    """n JPEGs of at most 96x72 with 1-4 boxes each; lines in the feeder's format."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        w, h = int(rng.randint(64, 97)), int(rng.randint(48, 73))
        path = str(folder / ('img_%d.jpg' % i))
        base = rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]).save(path, quality=85)
        parts = ['%d' % i, path, '%d' % w, '%d' % h]
        for _ in range(int(rng.randint(1, 5))):
            x0, y0 = rng.uniform(0, w * 0.5), rng.uniform(0, h * 0.5)
            parts += ['%d' % rng.randint(0, 80), '%.1f' % x0, '%.1f' % y0, '%.1f' % (x0 + rng.uniform(8, w * 0.45)),
                      '%.1f' % (y0 + rng.uniform(8, h * 0.45))]
        lines.append(' '.join(parts))
    return lines


def _epoch(feeder, epoch):
    out = []
    for b in feeder.epoch(epoch):
        out.append((b.image_ids, list(b.img_size), [t.cpu() for t in (b.images, b.boxes, b.labels, b.counts) + tuple(b.y_true)]))
    return out


def _same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for (ids_a, size_a, ts_a), (ids_b, size_b, ts_b) in zip(a, b):
        assert list(ids_a) == list(ids_b) and size_a == size_b
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(ts_a, ts_b))


FEEDER_KINDS = {'train': dict(mode='train', use_mix_up=True, multi_scale=True, interval=2, letterbox_resize=True),
                'val': dict(mode='val', letterbox_resize=False)}


@pytest.mark.parametrize('kind', sorted(FEEDER_KINDS))
def test_cached_feeder_serves_the_uncached_batches_even_without_the_files(tmp_path, kind):
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = _write_small_set(tmp_path, 12)
    kw = dict(num_threads=3, prefetch=2, seed=4, **FEEDER_KINDS[kind])
    plain = Feeder(lines, 4, 80, [64, 64], COCO_ANCHORS, pixels='gpu', **kw)
    want = [_epoch(plain, e) for e in range(3)]
    plain.close()
    cached = Feeder(lines, 4, 80, [64, 64], COCO_ANCHORS, pixels='gpu', cache_bytes=64 << 20, **kw)
    _same(_epoch(cached, 0), want[0])
    first = cached.cache.stats()
    assert first['images'] == 12 and first['bytes_refused'] == 0 and first['misses'] >= 12
    assert first['bytes_used'] <= 64 << 20
    for line in lines:                              # from here on a decode is impossible
        open(line.split(' ')[1], 'wb').close()
    for e in (1, 2):
        _same(_epoch(cached, e), want[e])
    after = cached.cache.stats()
    assert after['misses'] == first['misses'] and after['hits'] > first['hits'] and after['images'] == 12
    cached.close()


def test_a_cache_that_holds_half_of_the_set_mixes_both_kinds(tmp_path):
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = _write_small_set(tmp_path, 12)
    total = sum(int(l.split(' ')[2]) * int(l.split(' ')[3]) * 3 for l in lines)
    kw = dict(num_threads=3, prefetch=2, seed=6, **FEEDER_KINDS['train'])
    plain = Feeder(lines, 4, 80, [64, 64], COCO_ANCHORS, pixels='gpu', **kw)
    want = [_epoch(plain, e) for e in range(2)]
    plain.close()
    held = []
    for run in range(2):
        half = Feeder(lines, 4, 80, [64, 64], COCO_ANCHORS, pixels='gpu', cache_bytes=total // 2, **kw)
        for e in range(2):
            _same(_epoch(half, e), want[e])
        st = half.cache.stats()
        assert 0 < st['images'] < 12 and st['bytes_used'] <= total // 2 and st['bytes_refused'] > 0
        assert st['hits'] > 0 and st['misses'] > 12             # epoch 1 decoded what the arena had no room for
        held.append(dict(half.cache.index))
        half.close()
    assert held[0] == held[1]


def test_a_cache_needs_the_device_pixel_path(tmp_path):
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = _write_small_set(tmp_path, 2)
    for kw in (dict(pixels='host'), dict(backend='process'), dict(backend='process', pixels='gpu')):
        with pytest.raises(ValueError):
            Feeder(lines, 2, 80, [64, 64], COCO_ANCHORS, cache_bytes=1 << 20, **kw)
    assert Feeder(lines, 2, 80, [64, 64], COCO_ANCHORS, pixels='gpu').cache_bytes == 0
