"""Cases for the affine warp (include/yolo355.h: y3_affine), shared by tests/test_affine_cpu.py (the numpy oracle
utils.data_aug.affine_warp against a brute-force loop and against the host build of csrc/y3_affine_px.h) and
tests/test_affine_gpu.py (the kernels against the oracle).

Two kinds of pixels: in the cases whose record moves whole pixels every input pixel is its own flat index (image, y, x, c) as
an exact float32 integer, so a pixel taken from the wrong place shows; the others hold arbitrary floats of [0, 1), so every
product and sum of the blend rounds.  Box rows at or behind an image's count hold plausible boxes, not zeros: a kernel that
ignored the counts would keep them.

Sizes (H, W) = (32, 32) and (64, 96); n = 1 and 3; kmax in {1, 64, 65, 70, 280}.  The two sets of 200 affine_draw records run
at 32 x 32 (one case of n = 200 each: the brute-force loop of the CPU suite walks every pixel in Python); at 64 x 96 twelve
records of either set stand in."""
import collections
import random

import numpy as np

MIN_SIDE, MIN_AREA, MAX_ASPECT = 2.0, 0.1, 20.0
FILL = float(np.float32(128) / np.float32(255))        # (what the feeder passes; any float would do)
ONE = 65536
MODEST, WIDEST = (10.0, 0.1, 0.5, 2.0), (45.0, 0.5, 0.9, 10.0)       # affine_draw ranges: degrees, translate, scale, shear
KMAXES = (1, 64, 65, 70, 280)

Case = collections.namedtuple('Case', 'images boxes labels counts records fill min_side min_area max_aspect')


def bits(v):
    return int(np.asarray(v, np.float32).view(np.int32))


def record(inverse, forward):
    """A record from the six Q16 integers and the six forward floats, written out (not shared with the code under test)."""
    return [int(v) for v in inverse] + [bits(v) for v in forward]


IDENTITY = record((ONE, 0, 0, 0, ONE, 0), (1, 0, 0, 0, 1, 0))


def shift(dx, dy):
    """out(x, y) = in(x - dx, y - dy), dx / dy in pixels (multiples of 1/256 are exact); boxes move by (+dx, +dy)."""
    return record((ONE, 0, -int(round(dx * ONE)), 0, ONE, -int(round(dy * ONE))), (1, 0, dx, 0, 1, dy))


def quarter_turn(side):
    """out(x, y) = in(y, side - 1 - x) on a square image: a pure permutation.  Forward: (sx, sy) -> (side - sy, sx)."""
    return record((0, ONE, 0, -ONE, 0, (side - 1) * ONE), (0, -1, side, 1, 0, 0))


def zoom(z):
    """Zoom by z about the origin of the continuous coordinates: source index u = (x + 0.5) / z - 0.5."""
    inv = ONE / z
    assert inv == int(inv) and (inv / 2 - ONE / 2) == int(inv / 2 - ONE / 2)
    return record((int(inv), 0, int(inv / 2 - ONE / 2), 0, int(inv), int(inv / 2 - ONE / 2)), (z, 0, 0, 0, z, 0))


def unique_pixels(n, h, w):
    total = n * h * w * 3
    assert total < 2 ** 24, "float32 holds integers exactly below 2^24"
    return np.arange(total, dtype=np.float32).reshape(n, h, w, 3)


def noise_pixels(n, h, w, seed):
    return np.random.RandomState(seed).random_sample((n, h, w, 3)).astype(np.float32)


def random_boxes(rng, count, w, h, exact=False):
    x0, y0 = rng.uniform(-0.2 * w, 0.8 * w, count), rng.uniform(-0.2 * h, 0.8 * h, count)
    bw, bh = rng.uniform(1, 0.7 * w, count), rng.uniform(1, 0.7 * h, count)
    b = np.stack([x0, y0, x0 + bw, y0 + bh, rng.choice([1.0, 0.75, 0.3125, 0.1], count)], axis=1)
    if exact:
        b[:, :4] = np.round(b[:, :4] * 4) / 4
    return b.astype(np.float32)


def fill_boxes(n, kmax, w, h, rng, per_image):
    """boxes / labels / counts for n images: per_image(i) -> (float [k, 5], count or None); rows behind are plausible."""
    boxes = np.zeros((n, kmax, 5), np.float32)
    labels = rng.randint(0, 80, (n, kmax)).astype(np.int32)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        boxes[i] = random_boxes(rng, kmax, w, h)
        mine, count = per_image(i)
        mine = np.asarray(mine, np.float32).reshape(-1, 5)[:kmax]
        boxes[i, :len(mine)] = mine
        counts[i] = len(mine) if count is None else count
    return boxes, labels, counts


def case_of(images, records, kmax, seed, per_image=None, **kw):
    n, h, w, _ = images.shape
    assert len(records) == n
    rng = np.random.RandomState(seed)
    per_image = per_image or (lambda i: (random_boxes(rng, rng.randint(0, kmax + 1), w, h), None))
    boxes, labels, counts = fill_boxes(n, kmax, w, h, rng, per_image)
    c = Case(images, boxes, labels, counts, np.asarray(records, np.int64), FILL, MIN_SIDE, MIN_AREA, MAX_ASPECT)
    return c._replace(**kw)


def drawn(prng, w, h, ranges):
    from yolov3_tensorflow_amd.utils.data_aug import affine_draw
    return affine_draw(prng, w, h, *ranges)


def threshold_boxes(w, h):
    """Boxes under the identity record with max_aspect = 4: [(box, kept)], on and off each rule (w, h >= 32)."""
    nan = float('nan')
    return [
        ((5, 5, 15, 12, 1.0), True),                    # whole
        ((-1, 5, 2, 12, 0.5), True),                    # clipped at the left border to exactly min_side
        ((-10, 5, 1.75, 12, 1.0), False),               # ... to under min_side
        ((5, h - 2, 11, h + 6, 1.0), True),             # clipped at the bottom border to exactly min_side (2 of 8: a quarter)
        ((5, h - 1.5, 11, h + 6, 1.0), False),          # ... to under min_side
        ((-30, 5, 2.5, 12, 1.0), False),                # 2.5 x 7 left of 32.5 x 7: under min_area, nothing else fails
        ((-10, 5, 2.5, 12, 1.0), True),                 # 2.5 x 7 left of 12.5 x 7: a fifth
        ((5, 5, 14, 7, 1.0), False),                    # 9 x 2: wider than max_aspect = 4 times its height
        ((5, 5, 13, 7, 1.0), True),                     # 8 x 2: exactly max_aspect
        ((5, 5, 7, 14, 1.0), False),                    # 2 x 9: taller than max_aspect times its width
        ((w - 3, 3, w + 9, 9, 0.25), True),             # clipped at the right border: 3 x 6 of 12 x 6 left
        ((5, 5, 9, 9, nan), True),                      # the weight is carried, whatever it is
        ((nan, 5, 9, 9, 1.0), False),                   # a NaN corner is dropped
        ((5, nan, 9, 9, 1.0), False),
    ]


def all_cases(h, w):
    """name -> Case at one image size."""
    cases = collections.OrderedDict()
    prng = random.Random(1000 * h + w)
    # ---- records that move whole pixels, on unique pixels
    whole = [('identity', IDENTITY), ('shift_+3_-2', shift(3, -2)), ('shift_-5_+4', shift(-5, 4)), ('zoom_half', zoom(0.5)),
             ('outside_right', record((ONE, 0, 1 << 30, 0, ONE, 0), (1, 0, -16384, 0, 1, 0))),
             ('outside_above', record((ONE, 0, 0, 0, ONE, -(1 << 30)), (1, 0, 0, 0, 1, 16384))),
             ('extreme_ia', record((1 << 20, 0, 0, 0, 1 << 20, 0), (0.0625, 0, 0, 0, 0.0625, 0))),
             ('extreme_negative', record((-(1 << 20), -(1 << 20), (w - 1) << 20, 1 << 20, -(1 << 20), (h - 1) << 16),
                                         (-0.03125, -0.03125, 1, 0.03125, -0.03125, 2)))]
    if h == w:
        whole.append(('quarter_turn', quarter_turn(h)))
    for j, (name, rec) in enumerate(whole):
        cases[name] = case_of(unique_pixels(1, h, w), [rec], 17, seed=j)
    # ---- records that blend, on noise
    blend = [('shift_half', shift(0.5, 0.5)), ('zoom_2', zoom(2.0)),
             ('straddle_left_top', shift(0.5, 0.25)), ('straddle_right_bottom', shift(-0.5, -0.75)),
             ('negative_sx', record((ONE, 0, -1, 0, ONE, -1), (1, 0, 0, 0, 1, 0))),              # SX = -1 at x = 0: u0 = -1, fx = 255
             ('negative_sx_far', record((ONE, 0, -3 * ONE - 257, 0, ONE, -ONE - 1), (1, 0, 3, 0, 1, 1))),
             ('fraction_255', record((ONE, 0, 255 << 8, 0, ONE, 255 << 8), (1, 0, -1, 0, 1, -1))),
             ('fraction_x255_y0', record((ONE, 0, 255 << 8, 0, ONE, 0), (1, 0, -1, 0, 1, 0))),
             ('fraction_x0_y255', record((ONE, 0, 0, 0, ONE, (255 << 8) + 255), (1, 0, 0, 0, 1, -1)))]
    for j, (name, rec) in enumerate(blend):
        cases[name] = case_of(noise_pixels(1, h, w, 40 + j), [rec], 17, seed=20 + j)
    # ---- every (n, kmax) under drawn records
    for n in (1, 3):
        for kmax in KMAXES:
            recs = [drawn(prng, w, h, MODEST if (i + kmax) % 2 else WIDEST) for i in range(n)]
            cases['drawn_n%d_k%d' % (n, kmax)] = case_of(noise_pixels(n, h, w, 100 * n + kmax), recs, kmax, seed=100 * n + kmax)
    for name, ranges in (('modest', MODEST), ('widest', WIDEST)):
        many = 200 if h * w <= 1024 else 12
        recs = [drawn(prng, w, h, ranges) for _ in range(many)]
        cases['draws_%s_n%d' % (name, many)] = case_of(noise_pixels(many, h, w, 7), recs, 5, seed=len(name))
    # ---- boxes
    rng = np.random.RandomState(5)
    full = lambda count: (lambda i: (random_boxes(rng, 70, w, h), count))
    cases['counts_0_kmax_beyond'] = case_of(noise_pixels(3, h, w, 8), [shift(1.5, -2.25), drawn(prng, w, h, MODEST), zoom(2.0)], 70,
                                            seed=8, per_image=lambda i: (random_boxes(rng, 70, w, h), (0, 70, 75)[i]))
    cases['counts_negative'] = case_of(noise_pixels(1, h, w, 9), [IDENTITY], 17, seed=9, per_image=full(-3))
    thresholds = [b for b, _ in threshold_boxes(w, h)]
    cases['thresholds_k17'] = case_of(unique_pixels(1, h, w), [IDENTITY], 17, seed=10, per_image=lambda i: (thresholds, None),
                                      max_aspect=4.0)
    cases['thresholds_n3_k70'] = case_of(unique_pixels(3, h, w), [IDENTITY] * 3, 70, seed=11,
                                         per_image=lambda i: (thresholds if i != 1 else thresholds[::-1], None), max_aspect=4.0)

    def left_of_the_image(i):
        b = random_boxes(rng, 17, w, h)
        b[:, [0, 2]] -= np.float32(2 * w)
        return b, None
    cases['all_dropped'] = case_of(noise_pixels(1, h, w, 12), [IDENTITY], 17, seed=12, per_image=left_of_the_image)
    c = case_of(noise_pixels(3, h, w, 13), [shift(0.25, 0.25)] * 3, 17, seed=13)
    c.boxes[1, :, [0, 2]] -= np.float32(2 * w)
    c.counts[:] = (9, 17, 11)
    cases['one_image_all_dropped'] = c

    # full images of small boxes well inside: nearly all are kept, so every chunk of 64 writes behind what the chunks before
    # it kept, and kept boxes lie on both sides of every 64-boundary
    def dense(kmax):
        def per(i):
            x0, y0 = 2 + rng.randint(0, 4 * (w - 8), kmax) / 4., 2 + rng.randint(0, 4 * (h - 8), kmax) / 4.
            side = rng.choice([1.75, 2.0, 2.5, 3.0], (2, kmax), p=[0.02, 0.38, 0.3, 0.3])
            return np.stack([x0, y0, x0 + side[0], y0 + side[1], np.ones(kmax)], axis=1), None
        return per
    for kmax in (70, 280):
        cases['dense_n2_k%d' % kmax] = case_of(noise_pixels(2, h, w, kmax), [IDENTITY, shift(1, 0.5)], kmax, seed=kmax,
                                               per_image=dense(kmax))
    return cases


def guard_case():
    """The guard-band case: 2 images of 64 x 96 with kmax 17, one image full; the first record reads the last row and column
    of its input and taps beyond all four borders, the second is a drawn one."""
    prng = random.Random(77)
    case = case_of(noise_pixels(2, 64, 96, 77), [shift(-0.5, -0.5), drawn(prng, 96, 64, WIDEST)], 17, seed=77)
    case.counts[1] = 17
    return case


def feeder_set(tmp_path, n, classes=80, seed=5):
    """n JPEGs of about 320 x 240 with one to three boxes of at least 90 px a side: at 96 x 64 none of them comes near a
    threshold of the warp's box rule under the identity (tests/test_affine_cpu.py holds that for this very set and the feeder tests' seed)."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        w, h = int(rng.randint(280, 360)), int(rng.randint(200, 280))
        path = str(tmp_path / ('img_%d.jpg' % i))
        base = rng.randint(0, 256, (h // 8, w // 8, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]).save(path, quality=85)
        parts = ['%d' % i, path, '%d' % w, '%d' % h]
        for _ in range(int(rng.randint(1, 4))):
            x0, y0 = rng.uniform(0, w * 0.4), rng.uniform(0, h * 0.4)
            parts += ['%d' % rng.randint(0, classes), '%.1f' % x0, '%.1f' % y0, '%.1f' % (x0 + rng.uniform(90, w * 0.55)),
                      '%.1f' % (y0 + rng.uniform(90, h * 0.55))]
        lines.append(' '.join(parts))
    return lines


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
# test_guard_bands_gpu.py holds every entry point with a pointer argument against its table (TABLE / EXCLUDED).  y3_affine is
# added to that table from here, as mosaic_cases.py, iou_loss_cases.py and ema_cases.py add theirs: this module is imported
# whenever the suite is collected (tests/test_affine_cpu.py imports it).  tests/test_affine_gpu.py runs the entry through that
# module's own test.
def _register_guard_band_entry():
    import ctypes
    import torch
    import test_guard_bands_gpu as TG
    if any('y3_affine' in e.covers for e in TG.TABLE):
        return

    def affine(g):
        from yolov3_tensorflow_amd.utils.data_aug import affine_warp
        case = guard_case()
        n, h, w, _ = case.images.shape
        kmax = case.boxes.shape[1]
        sb = g.L.y3_affine_scratch_bytes(n)
        assert sb > 0
        recs = np.ascontiguousarray(case.records.astype(np.int32))
        outputs = ['out_images', 'out_boxes', 'out_labels', 'out_counts']
        specs = [TG.IN('in_images', case.images, align=4), TG.IN('in_boxes', case.boxes, align=4),
                 TG.IN('in_labels', case.labels.astype(np.int32), align=4), TG.IN('in_counts', case.counts.astype(np.int32), align=4),
                 TG.OUT('out_images', (n, h, w, 3), align=4), TG.OUT('out_boxes', (n, kmax, 5), align=4),
                 TG.OUT('out_labels', (n, kmax), dtype=torch.int32, align=4), TG.OUT('out_counts', (n,), dtype=torch.int32, align=4),
                 TG.S('scratch', sb, align=16)]

        def call(a):
            t = lambda k: TG.P(a[k])
            g('y3_affine', g.ctx, t('in_images'), t('in_boxes'), t('in_labels'), t('in_counts'), n, kmax, h, w,
              recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), case.fill, case.min_side, case.min_area, case.max_aspect,
              *[t(k) for k in outputs], t('scratch'), ctypes.c_size_t(sb))

        def verify(o):
            want = affine_warp(case.images, case.boxes, case.labels, case.counts, case.records, case.fill, case.min_side,
                               case.min_area, case.max_aspect)
            assert_same([o[k].numpy() for k in outputs], want, 'guarded')
        return TG.run_of(specs, call, outputs, verify)

    TG.entry('affine-2x64x96-k17', ('y3_affine',), affine)
    # (ema_cases.py: when this module is imported before pytest has read test_guard_bands' parametrize mark, whose list of ids
    # was made when that module was imported, the new entry needs its id there; imported later, nothing changes)
    for mark in getattr(TG.test_guard_bands, 'pytestmark', []):
        if mark.name == 'parametrize' and mark.args[1] is TG.TABLE and isinstance(mark.kwargs.get('ids'), list):
            ids = mark.kwargs['ids']
            ids.extend(e.id for e in TG.TABLE[len(ids):])


_register_guard_band_entry()
