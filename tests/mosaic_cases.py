"""Cases for the mosaic composition (include/yolo355.h: y3_mosaic), shared by tests/test_mosaic_cpu.py (the numpy oracle
utils.data_aug.mosaic4 against a brute-force loop and against the host build of csrc/y3_mosaic_px.h) and
tests/test_mosaic_gpu.py (the kernels against the oracle).

Every input pixel is its own flat index (sample, y, x, c) as an exact float32 integer, so a pixel copied from the wrong
place shows.  Box rows at or behind a sample's count hold plausible boxes, not zeros: a kernel that ignored the counts would
keep them.  Coordinates are multiples of 1/4 (exact in float32) except in the 'random' cases, which also carry arbitrary
floats."""
import collections
import random

import numpy as np

MIN_SIDE, MIN_VISIBLE = 2.0, 0.25

Case = collections.namedtuple('Case', 'images boxes labels counts records min_side min_visible')


def unique_pixels(samples, h, w):
    total = samples * h * w * 3
    assert total < 2 ** 24, "float32 holds integers exactly below 2^24"
    return np.arange(total, dtype=np.float32).reshape(samples, h, w, 3)


def tiles(record, w, h):
    """(tx, ty, tw, th, ox, oy) for q = 0..3, written out from the rule (not shared with the code under test)."""
    cx, cy = record[0], record[1]
    return [(0, 0, cx, cy, record[2], record[3]), (cx, 0, w - cx, cy, record[4], record[5]),
            (0, cy, cx, h - cy, record[6], record[7]), (cx, cy, w - cx, h - cy, record[8], record[9])]


def record_with(w, h, cx, cy, where):
    """A record with every offset at 0 ('zero'), at its maximum ('max') or alternating ('mixed')."""
    rec = [cx, cy]
    for q, (tw, th) in enumerate([(cx, cy), (w - cx, cy), (cx, h - cy), (w - cx, h - cy)]):
        hi = {'zero': (0, 0), 'max': (w - tw, h - th), 'mixed': ((w - tw) * (q & 1), (h - th) * (1 - (q & 1)))}[where]
        rec += [hi[0], hi[1]]
    return rec


def random_record(prng, w, h):
    """Any valid record (the whole validity range, wider than what mosaic_draw draws)."""
    cx, cy = prng.randint(1, w - 1), prng.randint(1, h - 1)
    rec = [cx, cy]
    for tw, th in [(cx, cy), (w - cx, cy), (cx, h - cy), (w - cx, h - cy)]:
        rec += [prng.randint(0, w - tw), prng.randint(0, h - th)]
    return rec


def _random_boxes(rng, count, w, h, exact=True):
    x0, y0 = rng.uniform(-0.2 * w, 0.8 * w, count), rng.uniform(-0.2 * h, 0.8 * h, count)
    bw, bh = rng.uniform(1, 0.7 * w, count), rng.uniform(1, 0.7 * h, count)
    b = np.stack([x0, y0, x0 + bw, y0 + bh, rng.choice([1.0, 0.75, 0.3125, 0.1], count)], axis=1)
    if exact:
        b[:, :4] = np.round(b[:, :4] * 4) / 4
    return b.astype(np.float32)


def _fill(n, kmax, w, h, rng, per_sample):
    """boxes / labels / counts for 4n samples: per_sample(s) -> float [k, 5] (k <= kmax); the rows behind are plausible."""
    boxes = np.zeros((4 * n, kmax, 5), np.float32)
    labels = rng.randint(0, 80, (4 * n, kmax)).astype(np.int32)
    counts = np.zeros(4 * n, np.int32)
    for s in range(4 * n):
        boxes[s] = _random_boxes(rng, kmax, w, h)
        mine = np.asarray(per_sample(s), np.float32).reshape(-1, 5)[:kmax]
        boxes[s, :len(mine)] = mine
        counts[s] = len(mine)
    return boxes, labels, counts


def random_case(h, w, n, kmax, seed, exact=False):
    rng, prng = np.random.RandomState(seed), random.Random(seed)
    records = [random_record(prng, w, h) for _ in range(n)]
    boxes, labels, counts = _fill(n, kmax, w, h, rng, lambda s: _random_boxes(rng, rng.randint(0, kmax + 1), w, h, exact))
    return Case(unique_pixels(4 * n, h, w), boxes, labels, counts, np.asarray(records, np.int32), MIN_SIDE, MIN_VISIBLE)


def threshold_boxes(tile, tw_min=8):
    """Boxes placed against the window of one tile (tw, th >= 8): [(box, kept)], on and just off each threshold."""
    _, _, tw, th, ox, oy = tile
    assert tw >= tw_min and th >= tw_min
    x, y = float(ox), float(oy)
    return [
        ((x + 1, y + 1, x + 5, y + 4, 1.0), True),                  # whole
        ((x - 3, y - 2, x + 3, y + 2, 0.5), True),                  # clipped on two sides: 3 x 2 of 6 x 4 left
        ((x - 3, y + 1, x + 2, y + 5, 1.0), True),                  # clipped width exactly min_side
        ((x - 3, y + 1, x + 1.75, y + 5, 1.0), False),              # ... just below it
        ((x + 1, y - 3, x + 5, y + 2, 1.0), True),                  # clipped height exactly min_side
        ((x + 1, y - 3, x + 5, y + 1.75, 1.0), False),              # ... just below it
        ((x - 6, y + 1, x + 2, y + 4, 0.25), True),                 # visible exactly min_visible of the area (2 of 8 wide)
        ((x - 6.25, y + 1, x + 2, y + 4, 0.25), False),             # ... just below it
        ((x - 6, y - 6, x + 2, y + 2, 1.0), False),                 # both sides on min_side, but 4 of 64 visible
        ((x - 9, y + 1, x, y + 4, 1.0), False),                     # touches the window: nothing left
        ((x + tw - 2, y + th - 2, x + tw + 1, y + th + 1, 1.0), True),      # the far corner: 2 x 2 of 3 x 3 left
        ((x + 1, y + 1, x + 3, y + 3, float('nan')), True),         # the weight is carried, whatever it is
        ((float('nan'), y + 1, x + 5, y + 4, 1.0), False),          # a NaN corner is dropped
    ]


def threshold_case(h, w, n, kmax):
    assert kmax >= 13
    rng = np.random.RandomState(3)
    records = [record_with(w, h, w // 2 + 3, h // 2 - 5, 'mixed') for _ in range(n)]
    per = lambda s: [b for b, _ in threshold_boxes(tiles(records[s // 4], w, h)[s % 4])]
    boxes, labels, counts = _fill(n, kmax, w, h, rng, per)
    return Case(unique_pixels(4 * n, h, w), boxes, labels, counts, np.asarray(records, np.int32), MIN_SIDE, MIN_VISIBLE)


def all_cases(h, w):
    """name -> Case at one image size (w a multiple of 32)."""
    cases = collections.OrderedDict()
    for n in (1, 3):
        for kmax in (1, 17, 70):      # 4 * 70 = 280 candidates: more than four chunks of 64
            cases['random_n%d_k%d' % (n, kmax)] = random_case(h, w, n, kmax, seed=100 * n + kmax)
    cases['random_exact_n3_k17'] = random_case(h, w, 3, 17, seed=9, exact=True)
    cases['thresholds_n1_k17'] = threshold_case(h, w, 1, 17)
    cases['thresholds_n3_k70'] = threshold_case(h, w, 3, 70)
    # full samples of small boxes inside their windows: nearly all of the 280 candidates are kept, so every chunk of 64 writes
    # behind what the chunks before it kept
    rng = np.random.RandomState(31)
    records = [record_with(w, h, w // 2 - 1, h // 2 + 2, 'mixed'), record_with(w, h, w // 2 + 5, h // 2 - 2, 'max')]

    def dense(s):
        _, _, tw, th, ox, oy = tiles(records[s // 4], w, h)[s % 4]
        x0, y0 = ox + rng.randint(0, 4 * (tw - 3), 70) / 4., oy + rng.randint(0, 4 * (th - 3), 70) / 4.
        side = rng.choice([1.75, 2.0, 2.5, 3.0], (2, 70), p=[0.1, 0.3, 0.3, 0.3])
        return np.stack([x0, y0, x0 + side[0], y0 + side[1], np.ones(70)], axis=1)
    boxes, labels, counts = _fill(2, 70, w, h, rng, dense)
    cases['dense_n2_k70'] = Case(unique_pixels(8, h, w), boxes, labels, counts, np.asarray(records, np.int32), MIN_SIDE, MIN_VISIBLE)
    # an image whose four samples hold no box, between two that do
    c = random_case(h, w, 3, 17, seed=21)
    c.counts[4:8] = 0
    cases['count_zero_image'] = c
    # every box dropped: all of them lie left of / above every window that can be cut (negative coordinates)
    c = random_case(h, w, 1, 17, seed=22)
    c.boxes[:, :, [0, 2]] -= np.float32(2 * w)
    c.counts[:] = 17
    cases['all_dropped'] = c
    # the centre at both extremes, offsets at 0 and at their maximum; an odd centre puts the tile border inside a 16-byte group
    for name, (cx, cy) in (('centre_min', (1, 1)), ('centre_max', (w - 1, h - 1)), ('centre_odd', (w // 2 + 1, h // 2 - 3))):
        for where in ('zero', 'max', 'mixed'):
            c = random_case(h, w, 1, 17, seed=23, exact=True)
            cases['%s_offsets_%s' % (name, where)] = c._replace(records=np.asarray([record_with(w, h, cx, cy, where)], np.int32))
    return cases


def guard_case():
    """The guard-band case: 2 outputs of 64 x 96 with kmax 17, one sample full (the last row of an input is read)."""
    case = random_case(64, 96, 2, 17, seed=77)
    case.counts[3] = 17
    return case


def assert_same(got, want, what=''):
    """Bit-identical images, boxes, labels, counts (NaN weights included: compared as bytes)."""
    for name, g, w_ in zip(('images', 'boxes', 'labels', 'counts'), got, want):
        g, w_ = np.ascontiguousarray(g), np.ascontiguousarray(w_)
        assert g.shape == w_.shape, (what, name, g.shape, w_.shape)
        if name in ('images', 'boxes'):
            assert g.dtype == w_.dtype == np.float32, (what, name, g.dtype, w_.dtype)
            same = g.view(np.uint32) == w_.view(np.uint32)
        else:
            same = g.astype(np.int64) == w_.astype(np.int64)
        assert same.all(), '%s: %s differ at %s' % (what, name, np.argwhere(~same)[:5].tolist())


# ---- the guard-band table -------------------------------------------------------------------------------------------------
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  y3_mosaic is
# added to that table from here, as iou_loss_cases.py and ema_cases.py add theirs: this module is imported whenever the suite
# is collected.  tests/test_mosaic_gpu.py runs the entry through that module's own test.
def _register_guard_band_entry():
    import ctypes
    import torch
    import test_guard_bands_gpu as TG
    if any('y3_mosaic' in e.covers for e in TG.TABLE):
        return

    def mosaic(g):
        from yolov3_tensorflow_amd.utils.data_aug import mosaic4
        case = guard_case()
        n4, h, w, _ = case.images.shape
        n, kmax = n4 // 4, case.boxes.shape[1]
        sb = g.L.y3_mosaic_scratch_bytes(n)
        assert sb > 0
        recs = np.ascontiguousarray(case.records, np.int32)
        outputs = ['out_images', 'out_boxes', 'out_labels', 'out_counts']
        specs = [TG.IN('in_images', case.images, align=16), TG.IN('in_boxes', case.boxes, align=4),
                 TG.IN('in_labels', case.labels.astype(np.int32), align=4), TG.IN('in_counts', case.counts.astype(np.int32), align=4),
                 TG.OUT('out_images', (n, h, w, 3), align=16), TG.OUT('out_boxes', (n, 4 * kmax, 5), align=4),
                 TG.OUT('out_labels', (n, 4 * kmax), dtype=torch.int32, align=4), TG.OUT('out_counts', (n,), dtype=torch.int32, align=4),
                 TG.S('scratch', sb, align=16)]

        def call(a):
            t = lambda k: TG.P(a[k])
            g('y3_mosaic', g.ctx, t('in_images'), t('in_boxes'), t('in_labels'), t('in_counts'), n, kmax, h, w,
              recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), case.min_side, case.min_visible, *[t(k) for k in outputs],
              t('scratch'), ctypes.c_size_t(sb))

        def verify(o):
            want = mosaic4(case.images, case.boxes, case.labels, case.counts, case.records, case.min_side, case.min_visible)
            assert_same([o[k].numpy() for k in outputs], want, 'guarded')
        return TG.run_of(specs, call, outputs, verify)

    TG.entry('mosaic-2x64x96-k17', ('y3_mosaic',), mosaic)
    # (ema_cases.py: when this module is imported before pytest has read test_guard_bands' parametrize mark, whose list of ids
    # was made when that module was imported, the new entry needs its id there; imported later, nothing changes)
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entry()
