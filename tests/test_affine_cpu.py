"""CPU tests of the affine warp (include/yolo355.h: y3_affine).  The numpy oracle utils.data_aug.affine_warp against
hand-written pins and against a brute-force loop; the host/device functions the kernels are made of (csrc/y3_affine_px.h) run
on the host (tests/affine_emul.cpp) against the oracle, bit for bit, over every case of tests/affine_cases.py; the draws; the
feeder's host half; the C interface; train.py's options.  tests/test_affine_gpu.py repeats the comparison with the kernels."""
import ctypes
import math
import os
import random
import re
import subprocess
import threading

import numpy as np
import pytest

import affine_cases as ac
from conftest import ROOT

SIZES = [(32, 32), (64, 96)]        # (H, W)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _pin_image():
    """One 8 x 12 image whose pixel at (y, x, c) is 3 (12 y + x) + c + 1 (no pixel is zero), and FILL = -7."""
    H, W = 8, 12
    idx = (np.arange(H)[:, None, None] * W + np.arange(W)[None, :, None]) * 3 + np.arange(3)[None, None, :] + 1
    return idx.astype(np.float32)[None], H, W


def test_affine_warp_pins_identity_shift_and_half_pixel():
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp
    images, H, W = _pin_image()
    boxes = np.array([[[2, 1, 7, 5, 0.5], [-3, -2, 4, 3, 1.0], [6, 4, 14, 10, 0.25]]], np.float32)
    labels, counts = np.array([[4, 7, 9]], np.int32), np.array([3], np.int32)
    warp = lambda rec: affine_warp(images, boxes, labels, counts, [rec], -7.0, 2.0, 0.1, 20.0)
    # identity: the input's bits, and the boxes clipped to the image
    out_images, out_boxes, out_labels, out_counts = warp(ac.IDENTITY)
    assert out_images.dtype == np.float32 and out_images.tobytes() == images.tobytes()
    np.testing.assert_array_equal(out_boxes[0], [[2, 1, 7, 5, 0.5], [0, 0, 4, 3, 1.0], [6, 4, 12, 8, 0.25]])
    np.testing.assert_array_equal(out_labels, [[4, 7, 9]])
    np.testing.assert_array_equal(out_counts, [3])
    # the integer shift (+3, -2): out(x, y) = in(x - 3, y + 2); the left 3 columns and the bottom 2 rows are fill
    out_images, out_boxes, out_labels, out_counts = warp(ac.shift(3, -2))
    want = np.full((H, W, 3), -7, np.float32)
    want[:H - 2, 3:] = images[0, 2:, :W - 3]
    np.testing.assert_array_equal(out_images[0], want)
    assert out_images[0, 0, 3, 0] == 3 * (12 * 2 + 0) + 1 and out_images[0, 5, 11, 2] == 3 * (12 * 7 + 8) + 3
    # boxes move by (+3, -2) and are clipped: the second keeps 7 x 1 -> under min_side, dropped
    np.testing.assert_array_equal(out_boxes[0], [[5, 0, 10, 3, 0.5], [9, 2, 12, 8, 0.25], [0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(out_labels, [[4, 9, 0]])
    np.testing.assert_array_equal(out_counts, [2])
    # the half-pixel shift: out(x, y) = ((in(x-1, y-1) + in(x, y-1)) / 2 + (in(x-1, y) + in(x, y)) / 2) / 2
    out_images = warp(ac.shift(0.5, 0.5))[0]
    p = lambda y, x, c=0: float(images[0, y, x, c]) if 0 <= y < H and 0 <= x < W else -7.0
    for y, x in ((3, 4), (1, 1), (7, 11)):
        assert out_images[0, y, x, 0] == 0.5 * (0.5 * p(y - 1, x - 1) + 0.5 * p(y - 1, x)) + 0.5 * (0.5 * p(y, x - 1) + 0.5 * p(y, x))
    assert out_images[0, 3, 4, 0] == 0.25 * (82 + 85 + 118 + 121)
    assert out_images[0, 0, 0, 1] == 0.25 * (-7 - 7 - 7 + 2)                # three taps beyond the corner
    assert out_images[0, 0, 5, 2] == 0.5 * -7 + 0.25 * (15 + 18)            # the top border
    # a pure horizontal half-pixel shift: 0.5 p + 0.5 q
    out_images = warp(ac.shift(0.5, 0))[0]
    assert out_images[0, 2, 6, 0] == 0.5 * p(2, 5) + 0.5 * p(2, 6) == 0.5 * 88 + 0.5 * 91
    assert out_images[0, 2, 0, 0] == 0.5 * -7 + 0.5 * 73


def test_affine_warp_pins_quarter_turn_drop_rules_and_bad_records():
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp
    images, H, W = _pin_image()
    square = np.ascontiguousarray(images[:, :, :8])         # 8 x 8
    nan = float('nan')
    boxes = np.array([[
        [1, 2, 4, 7, 1.0],              # kept by both records below
        [-9, 1, 1.5, 6, 1.0],           # clips to 1.5 wide: under min_side
        [-30, 1, 2.5, 3.5, 1.0],        # 2.5 x 2.5 of 32.5 x 2.5 left: under min_area (1/13 < 0.1)
        [1, 1, 8, 3, 1.0],              # 7 x 2: beyond max_aspect = 3
        [nan, 1, 4, 4, 1.0],            # a NaN corner
        [2, 2, 5, 5, nan],              # a NaN weight is carried
    ]], np.float32)
    labels, counts = np.arange(6, dtype=np.int32)[None] + 10, np.array([6], np.int32)
    _, out_boxes, out_labels, out_counts = affine_warp(square, boxes, labels, counts, [ac.IDENTITY], -7.0, 2.0, 0.1, 3.0)
    assert out_counts.tolist() == [2] and out_labels.tolist() == [[10, 15, 0, 0, 0, 0]]
    np.testing.assert_array_equal(out_boxes[0, 0], [1, 2, 4, 7, 1.0])
    assert out_boxes[0, 1, :4].tolist() == [2, 2, 5, 5] and np.isnan(out_boxes[0, 1, 4]) and not out_boxes[0, 2:].any()
    # the quarter turn: out(x, y) = in(y, 7 - x), a permutation; a box (x0, y0, x1, y1) becomes (8 - y1, x0, 8 - y0, x1)
    out_images, out_boxes, out_labels, out_counts = affine_warp(square, boxes, labels, counts, [ac.quarter_turn(8)], -7.0, 2.0,
                                                                0.1, 3.0)
    want = np.empty_like(square[0])
    for y in range(8):
        for x in range(8):
            want[y, x] = square[0, 7 - x, y]
    assert out_images[0].tobytes() == want.tobytes()
    assert out_images[0, 0, 0, 0] == square[0, 7, 0, 0] and out_images[0, 0, 7, 0] == square[0, 0, 0, 0]
    assert out_counts.tolist() == [2] and out_labels.tolist() == [[10, 15, 0, 0, 0, 0]]
    np.testing.assert_array_equal(out_boxes[0, 0], [1, 1, 6, 4, 1.0])
    assert out_boxes[0, 1, :4].tolist() == [3, 2, 6, 5]
    # a bad record raises, naming the image and the word
    two = np.concatenate([square, square])
    b2, l2, c2 = np.concatenate([boxes, boxes]), np.concatenate([labels, labels]), np.concatenate([counts, counts])
    bad = list(ac.IDENTITY)
    bad[1] = (1 << 20) + 1
    with pytest.raises(ValueError, match=r'image 1: word 1, ib=1048577 outside \[-1048576, 1048576\]'):
        affine_warp(two, b2, l2, c2, [ac.IDENTITY, bad], -7.0)
    bad = list(ac.IDENTITY)
    bad[5] = -(1 << 30) - 1
    with pytest.raises(ValueError, match=r'image 0: word 5, if=-1073741825 outside \[-1073741824, 1073741824\]'):
        affine_warp(two, b2, l2, c2, [bad, ac.IDENTITY], -7.0)
    bad = list(ac.IDENTITY)
    bad[8] = ac.bits(float('inf'))
    with pytest.raises(ValueError, match=r'image 1: word 8, fc is not finite'):
        affine_warp(two, b2, l2, c2, [ac.IDENTITY, bad], -7.0)


def brute_force(case):
    """The rule of include/yolo355.h as a per-pixel and per-box loop over Python integers and numpy float32 scalars (one
    pixel's three channels at a time): nothing shared with affine_warp."""
    f = np.float32
    n, H, W, _ = case.images.shape
    kmax = case.boxes.shape[1]
    images = np.full((n, H, W, 3), -1, np.float32)
    boxes, labels = np.zeros((n, kmax, 5), np.float32), np.zeros((n, kmax), np.int32)
    counts = np.zeros(n, np.int32)
    fill3 = np.full(3, case.fill, np.float32)
    weights = [(f(256 - k) / f(256), f(k) / f(256)) for k in range(256)]
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            ia, ib, ic, id_, ie, if_ = (int(v) for v in case.records[i][:6])
            src = case.images[i]
            for y in range(H):
                for x in range(W):
                    sx, sy = ia * x + ib * y + ic, id_ * x + ie * y + if_
                    u0, v0 = sx >> 16, sy >> 16             # Python's >> floors
                    (wx0, wx1), (wy0, wy1) = weights[(sx >> 8) & 255], weights[(sy >> 8) & 255]
                    taps = [src[v, u] if 0 <= u < W and 0 <= v < H else fill3
                            for u, v in ((u0, v0), (u0 + 1, v0), (u0, v0 + 1), (u0 + 1, v0 + 1))]
                    top = wx0 * taps[0] + wx1 * taps[1]
                    bot = wx0 * taps[2] + wx1 * taps[3]
                    images[i, y, x] = wy0 * top + wy1 * bot
            fa, fb, fc, fd, fe, ff = (np.asarray(int(v) & 0xffffffff, np.uint32).view(f) for v in case.records[i][6:12])
            at = 0
            for k in range(min(max(int(case.counts[i]), 0), kmax)):
                x0, y0, x1, y1, m = (f(v) for v in case.boxes[i, k])
                us, vs = [], []
                for cx, cy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
                    us.append(f(f(f(fa * cx) + f(fb * cy)) + fc))
                    vs.append(f(f(f(fd * cx) + f(fe * cy)) + ff))
                if any(np.isnan(v) for v in us + vs):
                    continue
                a0, a1, b0, b1 = max(min(us), f(0)), min(max(us), f(W)), max(min(vs), f(0)), min(max(vs), f(H))
                bw, bh = f(a1 - a0), f(b1 - b0)
                det = abs(f(f(fa * fe) - f(fb * fd)))
                need = f(f(case.min_area) * f(det * f(f(x1 - x0) * f(y1 - y0))))
                if bw >= f(case.min_side) and bh >= f(case.min_side) and f(bw * bh) >= need and \
                        bw <= f(f(case.max_aspect) * bh) and bh <= f(f(case.max_aspect) * bw):
                    boxes[i, at] = [a0, b0, a1, b1, m]
                    labels[i, at] = case.labels[i, k]
                    at += 1
            counts[i] = at
    return images, boxes, labels, counts


_ORACLE = {}


def oracle(size, name, case):
    """affine_warp of one case, computed once and shared by the tests of this module."""
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp
    if (size, name) not in _ORACLE:
        _ORACLE[(size, name)] = affine_warp(case.images, case.boxes, case.labels, case.counts, case.records, case.fill,
                                            case.min_side, case.min_area, case.max_aspect)
    return _ORACLE[(size, name)]


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_affine_warp_against_a_brute_force_loop(size):
    cases = ac.all_cases(*size)
    assert len(cases) >= 35
    for name, case in cases.items():
        ac.assert_same(oracle(size, name, case), brute_force(case), name)


def test_the_cases_hold_what_they_are_named_for():
    for size in SIZES:
        H, W = size
        cases = ac.all_cases(H, W)
        got = {name: oracle(size, name, case) for name, case in cases.items()}
        shapes = {(c.images.shape[0], c.boxes.shape[1]) for c in cases.values()}
        assert {(n, k) for n in (1, 3) for k in ac.KMAXES} <= shapes
        assert sum(len(c.records) for name, c in cases.items() if name.startswith('draws_')) == (400 if size == (32, 32) else 24)
        # identity and fx = fy = 0: the input's bits
        assert got['identity'][0].tobytes() == cases['identity'].images.tobytes()
        assert np.array_equal(got['shift_+3_-2'][0][0, :H - 2, 3:], cases['shift_+3_-2'].images[0, 2:, :W - 3])
        fill = np.float32(ac.FILL)
        assert (got['shift_+3_-2'][0][0, :, :3] == fill).all() and (got['shift_+3_-2'][0][0, H - 2:] == fill).all()
        if H == W:
            assert np.array_equal(got['quarter_turn'][0][0], cases['quarter_turn'].images[0][::-1].transpose(1, 0, 2))
        for name in ('outside_right', 'outside_above'):
            assert (got[name][0] == fill).all(), name        # every tap is fill, and fx = fy = 0
        assert (got['outside_right'][0] != cases['outside_right'].images).all()
        # the floor of a negative shift: at x = 0, y = 0 all four taps of 'negative_sx' but the last lie beyond the corner
        c = cases['negative_sx']
        w1, w0 = np.float32(255) / np.float32(256), np.float32(1) / np.float32(256)
        want = w0 * (w0 * fill + w1 * fill) + w1 * (w0 * fill + w1 * c.images[0, 0, 0])
        assert got['negative_sx'][0][0, 0, 0].tobytes() == want.astype(np.float32).tobytes()
        assert cases['extreme_ia'].records[0][0] == 1 << 20 and cases['extreme_negative'].records[0][0] == -(1 << 20)
        # boxes: the counts, the thresholds in order, the dropped images, the dense ones
        assert got['counts_0_kmax_beyond'][3][0] == 0 and cases['counts_0_kmax_beyond'].counts.tolist() == [0, 70, 75]
        assert got['counts_0_kmax_beyond'][3][1] > 0 and got['counts_0_kmax_beyond'][3][2] > 0
        assert got['counts_negative'][3].tolist() == [0]
        kept = [keep for _, keep in ac.threshold_boxes(W, H)]
        boxes, labels, counts = got['thresholds_k17'][1:]
        assert counts.tolist() == [sum(kept)] == [7]
        assert labels[0, :7].tolist() == cases['thresholds_k17'].labels[0, :len(kept)][np.asarray(kept)].tolist()
        assert got['thresholds_n3_k70'][3].tolist() == [7, 7, 7]
        assert got['all_dropped'][3].tolist() == [0] and cases['all_dropped'].counts.tolist() == [17]
        assert got['one_image_all_dropped'][3][1] == 0 and got['one_image_all_dropped'][3][0] > 0 and \
            got['one_image_all_dropped'][3][2] > 0
        assert 64 < int(got['dense_n2_k70'][3].min()) < 70              # kept boxes on both sides of the 64-boundary
        assert 3 * 64 < int(got['dense_n2_k280'][3].min()) < 280        # ... of every boundary


# ------------------------------------------------------------------------------------ the host/device functions, on the host
@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('affine_emul') / 'libaffine_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-Wall',
                           os.path.join(ROOT, 'tests', 'affine_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3af_emulate.restype = ctypes.c_int
    lib.y3af_emulate.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_float] * 4 + [
        ctypes.c_void_p] * 4
    return lib


def emulate(emul, case, records=None):
    n, H, W, _ = case.images.shape
    kmax = case.boxes.shape[1]
    ins = [np.ascontiguousarray(case.images, np.float32), np.ascontiguousarray(case.boxes, np.float32),
           np.ascontiguousarray(case.labels, np.int32), np.ascontiguousarray(case.counts, np.int32)]
    recs = np.ascontiguousarray(np.asarray(case.records if records is None else records, np.int64).astype(np.int32))
    outs = [np.full((n, H, W, 3), np.nan, np.float32), np.full((n, kmax, 5), np.nan, np.float32),
            np.full((n, kmax), -1, np.int32), np.full((n,), -1, np.int32)]
    p = lambda a: a.ctypes.data
    rc = emul.y3af_emulate(*[p(a) for a in ins], n, kmax, H, W, p(recs), case.fill, case.min_side, case.min_area,
                           case.max_aspect, *[p(a) for a in outs])
    return rc, outs


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_px_functions_against_affine_warp(emul, size):
    for name, case in ac.all_cases(*size).items():
        rc, outs = emulate(emul, case)
        assert rc == 0, name
        ac.assert_same(outs, oracle(size, name, case), name)


def test_px_record_check_is_the_validity_rule(emul):
    from yolov3_tensorflow_amd.utils.data_aug import affine_record_fault, AFFINE_WORDS
    case = ac.case_of(ac.noise_pixels(2, 8, 8, 1), [ac.IDENTITY, ac.IDENTITY], 3, seed=1)
    assert affine_record_fault(ac.IDENTITY, 8, 8) is None
    for word in range(6):
        bound = 1 << 30 if word in (2, 5) else 1 << 20
        for value, bad in ((bound, False), (-bound, False), (bound + 1, True), (-bound - 1, True)):
            rec = list(ac.IDENTITY)
            rec[word] = value
            rc, _ = emulate(emul, case, [ac.IDENTITY, rec])
            assert rc == (-(200 + word) if bad else 0), (word, value, rc)
            fault = affine_record_fault(rec, 8, 8)
            assert (fault is not None) == bad
            if bad:
                assert fault == 'word %d, %s=%d outside [%d, %d]' % (word, AFFINE_WORDS[word], value, -bound, bound)
    for word in range(6, 12):
        for value, bad in ((float('inf'), True), (float('-inf'), True), (float('nan'), True), (3.0e38, False), (-1e-45, False)):
            rec = list(ac.IDENTITY)
            rec[word] = ac.bits(value)
            rc, _ = emulate(emul, case, [rec, ac.IDENTITY])
            assert rc == (-(100 + word) if bad else 0), (word, value, rc)
            fault = affine_record_fault(rec, 8, 8)
            assert (fault is not None) == bad and (not bad or fault.startswith('word %d, %s is not finite' % (word, AFFINE_WORDS[word])))
    assert affine_record_fault(ac.IDENTITY, 4097, 8) is not None and affine_record_fault(ac.IDENTITY, 4096, 0) is not None
    assert affine_record_fault(ac.IDENTITY[:11], 8, 8) is not None


# ------------------------------------------------------------------------------------------------------------------ the draws
def test_affine_draw_is_deterministic_and_zero_ranges_give_the_identity():
    from yolov3_tensorflow_amd.utils.data_aug import affine_draw, AFFINE_IDENTITY
    draw = lambda seed: [affine_draw(random.Random(seed), 96, 64, *ac.MODEST) for _ in range(3)]
    assert draw(5) == draw(5) and draw(5) != draw(6)
    assert all(len(r) == 12 and all(isinstance(v, int) for v in r) for r in draw(5))
    for w, h in ((96, 64), (320, 320), (608, 416), (33, 7)):
        rec = affine_draw(random.Random(w), w, h, 0.0, 0.0, 0.0, 0.0)
        assert rec == list(AFFINE_IDENTITY) == ac.IDENTITY
        assert rec[:6] == [65536, 0, 0, 0, 65536, 0]
        assert np.asarray(rec[6:], np.int32).view(np.float32).tolist() == [1, 0, 0, 0, 1, 0]
        assert affine_draw(random.Random(w), w, h) == rec
    # the order of the draws: angle, zoom, shear x, shear y, tx, ty
    prng, twin = random.Random(11), random.Random(11)
    rec = affine_draw(prng, 96, 64, 30.0, 0.2, 0.4, 5.0)
    angle, zoom = math.radians(twin.uniform(-30.0, 30.0)), twin.uniform(1.0 - 0.4, 1.0 + 0.4)
    shx, shy = math.tan(math.radians(twin.uniform(-5, 5))), math.tan(math.radians(twin.uniform(-5, 5)))
    tx, ty = twin.uniform(0.5 - 0.2, 0.5 + 0.2) * 96, twin.uniform(0.5 - 0.2, 0.5 + 0.2) * 64
    shear = np.array([[1, shx, 0], [shy, 1, 0], [0, 0, 1]])
    turn = np.array([[zoom * math.cos(angle), -zoom * math.sin(angle), 0], [zoom * math.sin(angle), zoom * math.cos(angle), 0],
                     [0, 0, 1]])
    move = lambda x, y: np.array([[1, 0, x], [0, 1, y], [0, 0, 1.0]])
    A = move(tx, ty) @ shear @ turn @ move(-48, -32)
    got = np.asarray(rec[6:], np.int32).view(np.float32)
    np.testing.assert_allclose(got, A[:2].reshape(-1), rtol=2.0 ** -23, atol=1e-12)
    inv = np.linalg.inv(A)
    inv[:2, 2] += 0.5 * (inv[:2, 0] + inv[:2, 1]) - 0.5
    assert np.abs(np.asarray(rec[:6]) / 65536.0 - inv[:2].reshape(-1)).max() <= 2.0 ** -17 + 1e-9
    assert prng.random() == twin.random()           # six draws, no more


def test_affine_draws_at_the_widest_ranges_are_valid_and_invert_the_forward_map():
    """10,000 draws at (45 degrees, 0.5, 0.9, 10 degrees) for 320 and 608 px: every record passes the validity rule, and the
    forward map applied to the source position of an output pixel returns to that pixel's centre within a derived bound.

    The bound, per axis.  Each Q16 coefficient is round(v * 65536) / 65536: off by at most 2^-17.  For a pixel 0 <= x < W,
    0 <= y < H the source index u = ia x + ib y + ic is therefore off by at most e = (x + y + 1) 2^-17 <= (W + H + 1) 2^-17,
    and so is v.  The test maps (u + 0.5, v + 0.5) forward in float64 with the record's float32 coefficients.  With the exact
    float64 map (fa .. ff) the exact source returns exactly to (x + 0.5, y + 0.5), so the output's x is off by at most
    (|fa| + |fb|) e  from the source error, plus  2^-24 (|fa| |su| + |fb| |sv| + |fc|)  from the cast of fa, fb, fc to
    float32 (relative error 2^-24 each; (su, sv) the source coordinates), plus the float64 rounding of the closed-form
    inverse and of this evaluation, for which 1e-9 px stands (coefficients up to ~11, coordinates up to ~2e4: below 1e-11).
    y likewise with fd, fe, ff."""
    from yolov3_tensorflow_amd.utils.data_aug import affine_draw, affine_record_fault
    for side in (320, 608):
        prng = random.Random(side)
        recs = [affine_draw(prng, side, side, *ac.WIDEST) for _ in range(10000)]
        assert all(affine_record_fault(r, side, side) is None for r in recs)
        recs = np.asarray(recs, np.int64)
        inv = recs[:, :6] / 65536.0
        fwd = (recs[:, 6:] & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64)
        assert len({tuple(r) for r in recs.tolist()}) == 10000
        rng = np.random.RandomState(side)
        for x, y in [(0, 0), (side - 1, 0), (0, side - 1), (side - 1, side - 1), (side // 2, side // 2)] + \
                [tuple(p) for p in rng.randint(0, side, (5, 2))]:
            su, sv = inv[:, 0] * x + inv[:, 1] * y + inv[:, 2] + 0.5, inv[:, 3] * x + inv[:, 4] * y + inv[:, 5] + 0.5
            e = (x + y + 1) * 2.0 ** -17
            assert e <= (2 * side + 1) * 2.0 ** -17
            for row, centre in ((0, x + 0.5), (3, y + 0.5)):
                a, b, c = fwd[:, row], fwd[:, row + 1], fwd[:, row + 2]
                bound = (np.abs(a) + np.abs(b)) * e + 2.0 ** -24 * (np.abs(a * su) + np.abs(b * sv) + np.abs(c)) + 1e-9
                off = np.abs(a * su + b * sv + c - centre)
                assert (off <= bound).all(), (side, x, y, row, float((off / bound).max()))


# ----------------------------------------------------------------------------------------------------- the feeder, host half only
def _flat_set(tmp_path, n=7):
    from PIL import Image
    rng = np.random.RandomState(8)
    lines = []
    for i in range(n):
        path = str(tmp_path / ('flat_%d.jpg' % i))
        Image.fromarray(rng.randint(0, 256, (64, 96, 3)).astype(np.uint8)).save(path, quality=90)
        x0, y0 = rng.uniform(0, 40), rng.uniform(0, 24)
        lines.append('%d %s 96 64 %d %.1f %.1f %.1f %.1f' % (i, path, i % 3, x0, y0, x0 + rng.uniform(10, 50), y0 + rng.uniform(10, 36)))
    return lines


ANCHORS = np.arange(18, dtype=np.float32).reshape(9, 2) + 5


def _host_half(f, epoch=0):
    from yolov3_tensorflow_amd import feeder
    got = []
    for size, ids, images, boxes, labels, counts, owner in f._host_batches(epoch, f._delivery(feeder._Buffers(), None), threading.Event()):
        got.append((list(size), list(ids), np.asarray(images).tobytes(), boxes.tobytes(), labels.tobytes(), counts.tobytes()))
        owner[0].give(None, owner[1])
    f.close()
    return got


def test_feeder_without_affine_is_the_parents_host_half(tmp_path):
    from yolov3_tensorflow_amd.feeder import Feeder
    lines = _flat_set(tmp_path)
    mk = lambda **kw: Feeder(lines, 3, 3, [96, 64], ANCHORS, mode='train', use_mix_up=True, num_threads=3, prefetch=2, seed=7,
                             backend='thread', pixels='host', **kw)
    for mosaic in (False, True):
        plain, none, on = mk(mosaic=mosaic), mk(mosaic=mosaic, affine=None), mk(mosaic=mosaic, affine=ac.MODEST)
        assert none.affine is None and on.affine == ac.MODEST
        want = plain._plan(1)
        assert str(none._plan(1)) == str(want) and str(on._plan(1)) == str(want)        # the plan's entries do not change
        assert all(len(e) == (5 if mosaic else 3) for e in want)
        batches = _host_half(plain, 1)
        assert len(batches) == 3 and _host_half(none, 1) == batches and _host_half(on, 1) == batches
    with pytest.raises(ValueError, match='train'):
        Feeder(lines, 3, 3, [96, 64], ANCHORS, mode='val', affine=ac.MODEST)
    with pytest.raises(ValueError, match='degrees'):
        Feeder(lines, 3, 3, [96, 64], ANCHORS, mode='train', affine=(1.0, 2.0))


def test_feeder_affine_records_depend_on_neither_workers_backend_nor_ranks():
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.data_aug import affine_draw, affine_record_fault
    lines = ['%d /nowhere/img_%d.jpg 100 80 1 10 10 50 50' % (i, i) for i in range(10)]
    mk = lambda **kw: Feeder(lines, 4, 3, [96, 64], ANCHORS, mode='train', multi_scale=True, use_mix_up=True, seed=3,
                             affine=ac.WIDEST, **kw)

    def records(f, epoch=2):
        return [f._affine_records(epoch, entry, f.affine) for entry in f._plan(epoch)]
    for mosaic in (False, True):
        whole = records(mk(mosaic=mosaic))
        assert [len(r) for r in whole] == [4, 4, 2] and len({tuple(r) for batch in whole for r in batch}) == 10
        plan = mk(mosaic=mosaic)._plan(2)
        assert all(affine_record_fault(r, e[1][0], e[1][1]) is None for e, batch in zip(plan, whole) for r in batch)
        # drawn from (key, slot) with _plan's key, at the batch's own size
        key = (3 * 1000003 + 2) * 100003 + 1
        assert whole[1][2] == affine_draw(random.Random('affine-record-%d-%d' % (key, 2)), plan[1][1][0], plan[1][1][1], *ac.WIDEST)
        assert records(mk(mosaic=mosaic, num_threads=1)) == whole == records(mk(mosaic=mosaic, num_threads=7))
        assert records(mk(mosaic=mosaic, backend='thread')) == whole == records(mk(mosaic=mosaic, backend='process'))
        assert records(mk(mosaic=mosaic), epoch=1) != whole
        r0, r1 = records(mk(mosaic=mosaic, rank=0, world=2)), records(mk(mosaic=mosaic, rank=1, world=2))
        for w_, p0, p1 in zip(whole, r0, r1):
            assert w_[0::2] == p0 and w_[1::2] == p1
    # a rank without a share of a short batch takes the batch's first entry, and its record
    short = Feeder(lines[:9], 4, 3, [96, 64], ANCHORS, mode='train', seed=3, affine=ac.WIDEST, rank=1, world=2)
    first = Feeder(lines[:9], 4, 3, [96, 64], ANCHORS, mode='train', seed=3, affine=ac.WIDEST, rank=0, world=2)
    assert short._plan(0)[2][2] == first._plan(0)[2][2] and len(short._plan(0)[2][2]) == 1
    assert short._affine_records(0, short._plan(0)[2], ac.WIDEST) == first._affine_records(0, first._plan(0)[2], ac.WIDEST)
    # the same mosaic records with and without affine: the two draw from generators of their own
    assert str(mk(mosaic=True)._plan(2)) == str(Feeder(lines, 4, 3, [96, 64], ANCHORS, mode='train', multi_scale=True,
                                                       use_mix_up=True, seed=3, mosaic=True)._plan(2))


def test_the_feeder_tests_set_has_no_box_near_a_rule_of_the_filter(tmp_path):
    """tests/test_affine_gpu.py compares a feeder with every range at zero against one without the warp, boxes included: under
    the identity record no box of its two batches, composed by mosaic or not, may be clipped or dropped.  The boxes are the
    host half's, so this needs no device."""
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.data_aug import affine_warp, mosaic4
    lines = ac.feeder_set(tmp_path, 8)
    for mosaic in (False, True):
        f = Feeder(lines, 4, 80, [96, 64], ANCHORS, mode='train', use_mix_up=True, num_threads=2, prefetch=2, seed=4,
                   mosaic=mosaic, backend='thread', pixels='host', affine=(0.0, 0.0, 0.0, 0.0))
        from yolov3_tensorflow_amd import feeder
        plan, seen = f._plan(0), 0
        batches = f._host_batches(0, f._delivery(feeder._Buffers(), None), threading.Event(), plan)
        for entry, (size, ids, images, boxes, labels, counts, owner) in zip(plan, batches):
            got = [np.asarray(images).copy(), boxes.copy(), labels.astype(np.int32), counts.astype(np.int32)]
            owner[0].give(None, owner[1])
            if mosaic:
                got = list(mosaic4(*got, entry[3], f.mosaic_min_side, f.mosaic_min_visible))
            records = f._affine_records(0, entry, f.affine)
            assert records == [ac.IDENTITY] * len(got[0])
            ac.assert_same(affine_warp(*got, records, 0.5, f.affine_min_side, f.affine_min_area, f.affine_max_aspect), got,
                           'mosaic=%d' % mosaic)
            seen += int(np.sum(got[3]))
        f.close()
        assert seen >= 8


def test_pad_fill_is_the_letterbox_padding_of_a_batch():
    """What the feeder passes as `fill`: the float32 a padded pixel holds in a delivered batch."""
    from yolov3_tensorflow_amd.utils import data_utils
    assert data_utils.PAD_VALUE == 128
    fill = data_utils.pad_fill()
    assert isinstance(fill, float) and np.float32(fill) == np.float32(128) / np.float32(255) and fill == ac.FILL
    padded, _, dw, dh = data_utils.letterbox_resize(np.zeros((10, 40, 3), np.uint8), 32, 32, interp=1)
    assert dh > 0 and (np.asarray(padded[0], np.float32) / 255. == np.float32(fill)).all()


# ------------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope='module')
def lib():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_abi_declares_prototypes_and_exports_both_symbols(lib):
    from yolov3_tensorflow_amd import _lib, build
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'yolo355.h')).read(), flags=re.S)
    for name in ('y3_affine', 'y3_affine_scratch_bytes'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES['y3_affine'][1]) == 20
    assert ('y3_affine.hip', ['-ffp-contract=off']) in build.SOURCES
    assert lib.y3_abi_version() == 5
    assert lib.y3_affine_scratch_bytes(0) == 0 and lib.y3_affine_scratch_bytes(-3) == 0
    assert lib.y3_affine_scratch_bytes(1) >= 48 and lib.y3_affine_scratch_bytes(64) >= 64 * 48
    sizes = [lib.y3_affine_scratch_bytes(n) for n in range(0, 200)] + [lib.y3_affine_scratch_bytes(16383)]
    assert sizes == sorted(sizes) and sizes[-1] >= 16383 * 48
    # a null context is refused before anything else is looked at; a negative n with a context-less call likewise
    rec = (ctypes.c_int32 * 12)(*[v if v < 2 ** 31 else v - 2 ** 32 for v in ac.IDENTITY])
    d = ctypes.c_void_p(256)
    assert lib.y3_affine(None, d, d, d, d, 1, 1, 32, 32, rec, 0.5, 2.0, 0.1, 20.0, d, d, d, d, d, 256) == _lib.Y3_EINVAL
    assert b'context' in lib.y3_last_error()
    assert lib.y3_affine(None, d, d, d, d, 0, 1, 32, 32, rec, 0.5, 2.0, 0.1, 20.0, d, d, d, d, d, 256) == _lib.Y3_EINVAL
    assert lib.y3_affine(None, d, d, d, d, -1, 1, 32, 32, rec, 0.5, 2.0, 0.1, 20.0, d, d, d, d, d, 256) == _lib.Y3_EINVAL


# ------------------------------------------------------------------------------------------------------------- train.py's options
def test_train_script_options_and_epoch_schedule():
    import train
    p = train.build_parser()
    args = p.parse_args([])
    assert (args.affine_degrees, args.affine_translate, args.affine_scale, args.affine_shear, args.affine_off_epochs) == (0, 0, 0, 0, 0)
    assert train.affine_ranges(args) is None
    assert not any(train.affine_in_epoch(args, e) for e in range(args.total_epoches))
    args = p.parse_args(['--affine_degrees', '10', '--affine_scale', '0.5', '--affine_off_epochs', '3', '--total_epoches', '10'])
    assert train.affine_ranges(args) == (10.0, 0.0, 0.5, 0.0)
    assert [train.affine_in_epoch(args, e) for e in range(10)] == [(10.0, 0.0, 0.5, 0.0)] * 7 + [None] * 3
    for flag in ('--affine_degrees', '--affine_translate', '--affine_scale', '--affine_shear'):     # any one switches it on
        assert train.affine_ranges(p.parse_args([flag, '0.25'])) is not None
    args = p.parse_args(['--affine_shear', '2', '--augment', 'false'])
    assert train.affine_ranges(args) is None and train.affine_in_epoch(args, 0) is None
    args = p.parse_args(['--affine_shear', '2', '--affine_off_epochs', '9', '--total_epoches', '4'])
    assert [train.affine_in_epoch(args, e) for e in range(4)] == [None] * 4
    # the schedule is what the epoch loop writes into the feeder's field, and the feeder reads it per epoch
    src = open(os.path.join(ROOT, 'train.py')).read()
    assert re.search(r'affine=affine_ranges\(args\)', src) and re.search(r'feeder\.affine = affine_in_epoch\(args, epoch\)', src)
    tool = open(os.path.join(ROOT, 'tools', 'feeder_rate.py')).read()
    assert "'--affine'" in tool and 'affine=AFFINE if affine else None' in tool
