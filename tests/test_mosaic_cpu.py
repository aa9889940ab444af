"""CPU tests of the mosaic composition (include/yolo355.h: y3_mosaic).  The numpy oracle utils.data_aug.mosaic4 against
hand-written pins and against a brute-force loop; the host/device functions the kernels are made of (csrc/y3_mosaic_px.h) run
on the host (tests/mosaic_emul.cpp) against the oracle, bit for bit, over every case of tests/mosaic_cases.py; the draws; the
feeder's plan; the C interface; train.py's options.  tests/test_mosaic_gpu.py repeats the comparison with the kernels."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mosaic_cases as mc
from conftest import ROOT

SIZES = [(32, 32), (64, 96)]        # (H, W)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_mosaic4_against_hand_written_pins():
    """One 8 x 12 output from four samples whose pixel at (s, y, x, c) is 1000 s + 3 (12 y + x) + c, and six boxes."""
    from yolov3_tensorflow_amd.utils.data_aug import mosaic4
    H, W = 8, 12
    idx = (np.arange(H)[:, None, None] * W + np.arange(W)[None, :, None]) * 3 + np.arange(3)[None, None, :]
    images = np.stack([1000 * s + idx for s in range(4)]).astype(np.float32)
    # cx, cy, then (ox, oy) of tiles 0..3: tile 1's oy and tile 2's ox are at their maxima (H - 3 and W - 5)
    record = [5, 3, 2, 1, 0, 5, 7, 0, 3, 2]
    nan = float('nan')
    boxes = np.array([
        [[3, 1.5, 6, 3.5, 1.0], [0, 0, 5, 3, 0.5]],         # sample 0, window [2,7) x [1,4): whole; clipped on two sides
        [[1, 4, 6, 6.5, 1.0], [1, 3, 4, 7, 1.0]],           # sample 1, window [0,7) x [5,8): 1.5 high (dropped); 2 high (kept)
        [[-4, 0, 9, 4, 1.0], [nan, nan, nan, nan, nan]],    # sample 2, window [7,12) x [0,5): 8 of 52 visible (dropped); no box
        [[-3, 3, 5, 6, 0.25], [1, 1, 9, 9, 1.0]],           # sample 3, window [3,10) x [2,7): 6 of 24 visible (kept); no box
    ], np.float32)
    labels = np.array([[4, 7], [1, 2], [5, 6], [9, 8]], np.int32)
    counts = np.array([2, 2, 1, 1], np.int32)
    out_images, out_boxes, out_labels, out_counts = mosaic4(images, boxes, labels, counts, [record], 2.0, 0.25)
    channel0 = np.array([
        [42, 45, 48, 51, 54, 1180, 1183, 1186, 1189, 1192, 1195, 1198],
        [78, 81, 84, 87, 90, 1216, 1219, 1222, 1225, 1228, 1231, 1234],
        [114, 117, 120, 123, 126, 1252, 1255, 1258, 1261, 1264, 1267, 1270],
        [2021, 2024, 2027, 2030, 2033, 3081, 3084, 3087, 3090, 3093, 3096, 3099],
        [2057, 2060, 2063, 2066, 2069, 3117, 3120, 3123, 3126, 3129, 3132, 3135],
        [2093, 2096, 2099, 2102, 2105, 3153, 3156, 3159, 3162, 3165, 3168, 3171],
        [2129, 2132, 2135, 2138, 2141, 3189, 3192, 3195, 3198, 3201, 3204, 3207],
        [2165, 2168, 2171, 2174, 2177, 3225, 3228, 3231, 3234, 3237, 3240, 3243],
    ], np.float32)
    assert out_images.shape == (1, H, W, 3) and out_images.dtype == np.float32
    for c in range(3):
        np.testing.assert_array_equal(out_images[0, :, :, c], channel0 + c)
    want_boxes = np.array([[1, 0.5, 4, 2.5, 1.0], [0, 0, 3, 2, 0.5], [6, 0, 9, 2, 1.0], [5, 4, 7, 7, 0.25],
                           [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    assert out_boxes.shape == (1, 8, 5) and out_boxes.dtype == np.float32
    np.testing.assert_array_equal(out_boxes[0], want_boxes)
    np.testing.assert_array_equal(out_labels, [[4, 7, 2, 9, 0, 0, 0, 0]])
    np.testing.assert_array_equal(out_counts, [4])
    # a bad record is refused with the image named
    with pytest.raises(ValueError, match='image 0: cx=0'):
        mosaic4(images, boxes, labels, counts, [[0] + record[1:]], 2.0, 0.25)


def brute_force(case):
    """The rule of include/yolo355.h as a per-pixel and per-box loop over numpy float32 scalars: nothing shared with mosaic4."""
    f = np.float32
    n4, H, W, _ = case.images.shape
    n, kmax = n4 // 4, case.boxes.shape[1]
    images = np.full((n, H, W, 3), -1, np.float32)
    boxes, labels = np.zeros((n, 4 * kmax, 5), np.float32), np.zeros((n, 4 * kmax), np.int32)
    counts = np.zeros(n, np.int32)
    for i in range(n):
        t = mc.tiles([int(v) for v in case.records[i]], W, H)
        cx, cy = int(case.records[i][0]), int(case.records[i][1])
        for y in range(H):
            for x in range(W):
                q = (1 if x >= cx else 0) + (2 if y >= cy else 0)
                tx, ty, _, _, ox, oy = t[q]
                images[i, y, x] = case.images[4 * i + q, y - ty + oy, x - tx + ox]
        at = 0
        for q in range(4):
            tx, ty, tw, th, ox, oy = t[q]
            wx0, wy0, wx1, wy1 = f(ox), f(oy), f(ox + tw), f(oy + th)
            for k in range(int(case.counts[4 * i + q])):
                x0, y0, x1, y1, m = (f(v) for v in case.boxes[4 * i + q, k])
                if any(np.isnan(v) for v in (x0, y0, x1, y1)):
                    continue
                a0, b0, a1, b1 = max(x0, wx0), max(y0, wy0), min(x1, wx1), min(y1, wy1)
                cw, ch = f(a1 - a0), f(b1 - b0)
                if cw >= f(case.min_side) and ch >= f(case.min_side) and \
                        f(cw * ch) >= f(f(case.min_visible) * f(f(x1 - x0) * f(y1 - y0))):
                    boxes[i, at] = [f(f(a0 - wx0) + f(tx)), f(f(b0 - wy0) + f(ty)), f(f(a1 - wx0) + f(tx)),
                                    f(f(b1 - wy0) + f(ty)), m]
                    labels[i, at] = case.labels[4 * i + q, k]
                    at += 1
        counts[i] = at
    return images, boxes, labels, counts


_ORACLE = {}


def oracle(size, name, case):
    """mosaic4 of one case, computed once and shared by the tests of this module."""
    from yolov3_tensorflow_amd.utils.data_aug import mosaic4
    if (size, name) not in _ORACLE:
        _ORACLE[(size, name)] = mosaic4(case.images, case.boxes, case.labels, case.counts, case.records, case.min_side,
                                        case.min_visible)
    return _ORACLE[(size, name)]


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_mosaic4_against_a_brute_force_loop(size):
    cases = mc.all_cases(*size)
    assert len(cases) >= 20
    for name, case in cases.items():
        mc.assert_same(oracle(size, name, case), brute_force(case), name)


def test_the_cases_hold_what_they_are_named_for():
    from yolov3_tensorflow_amd.utils.data_aug import mosaic_tiles
    for size in SIZES:
        H, W = size
        cases = mc.all_cases(H, W)
        got = {name: oracle(size, name, case) for name, case in cases.items()}
        assert got['all_dropped'][3].tolist() == [0] and cases['all_dropped'].counts.sum() == 68
        assert got['count_zero_image'][3][1] == 0 and got['count_zero_image'][3][0] > 0 and got['count_zero_image'][3][2] > 0
        assert 3 * 64 < int(got['dense_n2_k70'][3].min()) < 280      # every chunk of 64 candidates writes behind the earlier ones
        # the threshold boxes are kept and dropped as written beside them, in order
        case = cases['thresholds_n1_k17']
        kept = [keep for q in range(4) for _, keep in mc.threshold_boxes(mc.tiles(case.records[0].tolist(), W, H)[q])]
        assert got['thresholds_n1_k17'][3][0] == sum(kept) == 4 * 7
        assert [mosaic_tiles(case.records[0], W, H)[q] for q in range(4)] == mc.tiles(case.records[0].tolist(), W, H)
        recs = np.concatenate([c.records for c in cases.values()])
        assert recs[:, 0].min() == 1 and recs[:, 0].max() == W - 1 and recs[:, 1].min() == 1 and recs[:, 1].max() == H - 1
        assert any(r[0] % 4 for r in recs)                              # a tile border inside a 16-byte group of four floats


# ------------------------------------------------------------------------------------ the host/device functions, on the host
@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('mosaic_emul') / 'libmosaic_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-Wall',
                           os.path.join(ROOT, 'tests', 'mosaic_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3mo_emulate.restype = ctypes.c_int
    lib.y3mo_emulate.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float] + [
        ctypes.c_void_p] * 4
    return lib


def emulate(emul, case):
    n4, H, W, _ = case.images.shape
    n, kmax = n4 // 4, case.boxes.shape[1]
    ins = [np.ascontiguousarray(case.images, np.float32), np.ascontiguousarray(case.boxes, np.float32),
           np.ascontiguousarray(case.labels, np.int32), np.ascontiguousarray(case.counts, np.int32)]
    recs = np.ascontiguousarray(case.records, np.int32)
    outs = [np.full((n, H, W, 3), np.nan, np.float32), np.full((n, 4 * kmax, 5), np.nan, np.float32),
            np.full((n, 4 * kmax), -1, np.int32), np.full((n,), -1, np.int32)]
    p = lambda a: a.ctypes.data
    rc = emul.y3mo_emulate(*[p(a) for a in ins], n, kmax, H, W, p(recs), case.min_side, case.min_visible, *[p(a) for a in outs])
    return rc, outs


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_px_functions_against_mosaic4(emul, size):
    for name, case in mc.all_cases(*size).items():
        rc, outs = emulate(emul, case)
        assert rc == 0, name
        mc.assert_same(outs, oracle(size, name, case), name)


def test_px_record_check_is_the_validity_rule(emul):
    from yolov3_tensorflow_amd.utils.data_aug import mosaic_record_fault
    H, W = 32, 64
    case = mc.random_case(H, W, 2, 3, seed=1)
    top, zero = mc.record_with(W, H, 20, 9, 'max'), mc.record_with(W, H, 20, 9, 'zero')
    assert mosaic_record_fault(top, W, H) is None and mosaic_record_fault(zero, W, H) is None and min(top) > 0
    for good, bad_delta in ((top, 1), (zero, -1)):      # every offset: one past its maximum, one below zero; one inside either
        for at in range(2, 10):
            for delta in (-1, 1):
                rec = list(good)
                rec[at] += delta
                bad = delta == bad_delta
                rc, _ = emulate(emul, case._replace(records=np.asarray([good, rec], np.int32)))
                assert rc == (-3 if bad else 0), (at, delta, rc)
                assert (mosaic_record_fault(rec, W, H) is not None) == bad
    for cx, cy, bad in ((0, 9, True), (W, 9, True), (20, 0, True), (20, H, True), (1, 1, False), (W - 1, H - 1, False)):
        rec = [cx, cy] + zero[2:]
        rc, _ = emulate(emul, case._replace(records=np.asarray([rec, zero], np.int32)))
        assert rc == (-2 if bad else 0) and (mosaic_record_fault(rec, W, H) is not None) == bad


# ------------------------------------------------------------------------------------------------------------------ the draws
def test_mosaic_draw_is_deterministic_valid_and_reaches_its_extremes():
    from yolov3_tensorflow_amd.utils.data_aug import mosaic_draw, mosaic_record_fault
    assert [mosaic_draw(random.Random(5), 96, 64) for _ in range(3)] == [mosaic_draw(random.Random(5), 96, 64) for _ in range(3)]
    assert mosaic_draw(random.Random(5), 96, 64) != mosaic_draw(random.Random(6), 96, 64)
    for w, h in ((32, 32), (96, 64), (608, 608)):
        prng = random.Random(w + h)
        recs = [mosaic_draw(prng, w, h) for _ in range(3000)]
        assert all(len(r) == 10 and all(isinstance(v, int) for v in r) for r in recs)
        assert all(mosaic_record_fault(r, w, h) is None for r in recs)
        assert all(w // 4 <= r[0] <= w - w // 4 and h // 4 <= r[1] <= h - h // 4 for r in recs)
        if (w, h) == (32, 32):
            assert {8, 24} <= {r[0] for r in recs} and {8, 24} <= {r[1] for r in recs}
            assert any(r[2] == 0 for r in recs) and any(r[2] == w - r[0] for r in recs)         # ox0 at both ends
            assert any(r[9] == 0 for r in recs) and any(r[9] == r[1] for r in recs)             # oy3: th = h - cy, max = cy
    # the order of the draws: the centre first, then (ox, oy) tile by tile
    prng, twin = random.Random(11), random.Random(11)
    rec = mosaic_draw(prng, 96, 64)
    cx, cy = twin.randrange(24, 73), twin.randrange(16, 49)
    want = [cx, cy]
    for tw, th in ((cx, cy), (96 - cx, cy), (cx, 64 - cy), (96 - cx, 64 - cy)):
        want += [twin.randrange(0, 96 - tw + 1), twin.randrange(0, 64 - th + 1)]
    assert rec == want


# ------------------------------------------------------------------------------------------------------------- the feeder's plan
def _lines(n):
    return ['%d /nowhere/img_%d.jpg 100 80 1 10 10 50 50' % (i, i) for i in range(n)]


def test_feeder_plan_groups_four_per_slot_before_the_rank_split():
    from yolov3_tensorflow_amd.feeder import Feeder
    from yolov3_tensorflow_amd.utils.data_aug import mosaic_record_fault
    lines = _lines(10)
    anchors = np.arange(18, dtype=np.float32).reshape(9, 2) + 5
    mk = lambda **kw: Feeder(lines, 4, 3, [96, 64], anchors, mode='train', multi_scale=True, use_mix_up=True, seed=3, **kw)
    plain, whole = mk()._plan(2), mk(mosaic=True)._plan(2)
    assert len(mk(mosaic=True)) == len(mk()) == len(whole) == 3
    paired = 0
    for (b0, size0, entries), (b, size, groups, records, own) in zip(plain, whole):
        assert (b, size) == (b0, size0) and len(groups) == len(records) == len(own) == len(entries)
        for entry, group, rec, o in zip(entries, groups, records, own):
            assert len(group) == 4 and group[o] == entry            # the batch's own entry (a mix-up pair survives), somewhere
            assert all(g in lines for j, g in enumerate(group) if j != o)
            assert mosaic_record_fault(rec, size[0], size[1]) is None
            paired += isinstance(entry, list)
    assert paired > 0
    assert str(mk(mosaic=True)._plan(2)) == str(whole) and str(mk(mosaic=True)._plan(1)) != str(whole)
    assert len({o for e in whole for o in e[4]}) > 1 and len({tuple(r) for e in whole for r in e[3]}) == 10
    r0, r1 = mk(mosaic=True, rank=0, world=2)._plan(2), mk(mosaic=True, rank=1, world=2)._plan(2)
    for w_, p0, p1 in zip(whole, r0, r1):
        assert w_[:2] == p0[:2] == p1[:2]
        for part in (2, 3, 4):
            assert w_[part][0::2] == p0[part] and (w_[part][1::2] or w_[part][:1]) == p1[part]
    # the jobs: 4 n of them, sample 4 j + tile, every key its own
    f = mk(mosaic=True)
    jobs = f._jobs(2, whole[0])
    assert [j[0] for j in jobs] == [g for group in whole[0][2] for g in group] and len({j[4] for j in jobs}) == 16
    assert f._jobs(2, plain[0]) == [f._job(2, plain[0][0], j, line, plain[0][1]) for j, line in enumerate(plain[0][2])]
    # off: the parent's plan; the flag is read per epoch; only 'train' feeders take it
    assert str(mk(mosaic=False)._plan(2)) == str(plain)
    f.mosaic = False
    assert str(f._plan(2)) == str(plain)
    with pytest.raises(ValueError, match='train'):
        Feeder(lines, 4, 3, [96, 64], anchors, mode='val', mosaic=True)


def test_mosaic_lines_draws_three_lines_and_shuffles():
    from yolov3_tensorflow_amd.utils.data_utils import mosaic_lines
    lines = _lines(7)
    entries = [lines[0], [lines[1], lines[2]]]
    groups, own = mosaic_lines(entries, lines, random.Random(4))
    twin = random.Random(4)
    for entry, group, o in zip(entries, groups, own):
        want = [entry] + [lines[twin.randrange(7)] for _ in range(3)]
        order = list(range(4))
        twin.shuffle(order)
        assert group == [want[j] for j in order] and order[o] == 0


# ------------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope='module')
def lib():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_abi_declares_prototypes_and_exports_both_symbols(lib):
    from yolov3_tensorflow_amd import _lib, build
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'yolo355.h')).read(), flags=re.S)
    for name in ('y3_mosaic', 'y3_mosaic_scratch_bytes'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES['y3_mosaic'][1]) == 18
    assert ('y3_mosaic.hip', ['-ffp-contract=off']) in build.SOURCES
    assert lib.y3_abi_version() == 5
    assert lib.y3_mosaic_scratch_bytes(0) == 0 and lib.y3_mosaic_scratch_bytes(-3) == 0
    assert lib.y3_mosaic_scratch_bytes(1) >= 40 and lib.y3_mosaic_scratch_bytes(64) >= 64 * 40
    assert lib.y3_mosaic_scratch_bytes(64) <= lib.y3_mosaic_scratch_bytes(65)
    # a null context is refused before anything else is looked at
    rec = (ctypes.c_int32 * 10)(16, 16, 0, 0, 0, 0, 0, 0, 0, 0)
    d = ctypes.c_void_p(256)
    assert lib.y3_mosaic(None, d, d, d, d, 1, 1, 32, 32, rec, 2.0, 0.25, d, d, d, d, d, 256) == _lib.Y3_EINVAL
    assert b'context' in lib.y3_last_error()
    assert lib.y3_mosaic(None, d, d, d, d, 0, 1, 32, 32, rec, 2.0, 0.25, d, d, d, d, d, 256) == _lib.Y3_EINVAL


# ------------------------------------------------------------------------------------------------------------- train.py's options
def test_train_script_options_and_epoch_schedule():
    import train
    p = train.build_parser()
    args = p.parse_args([])
    assert args.mosaic is False and args.mosaic_off_epochs == 0
    assert not any(train.mosaic_in_epoch(args, e) for e in range(args.total_epoches))
    args = p.parse_args(['--mosaic', 'true', '--mosaic_off_epochs', '3', '--total_epoches', '10'])
    assert args.mosaic is True and args.mosaic_off_epochs == 3
    assert [train.mosaic_in_epoch(args, e) for e in range(10)] == [True] * 7 + [False] * 3
    args = p.parse_args(['--mosaic', 'true', '--total_epoches', '4'])
    assert [train.mosaic_in_epoch(args, e) for e in range(4)] == [True] * 4
    args = p.parse_args(['--mosaic', 'true', '--mosaic_off_epochs', '9', '--total_epoches', '4'])
    assert [train.mosaic_in_epoch(args, e) for e in range(4)] == [False] * 4
    # the schedule is what the epoch loop writes into the feeder's flag, and the feeder reads it per epoch
    src = open(os.path.join(ROOT, 'train.py')).read()
    assert re.search(r'feeder\.mosaic = mosaic_in_epoch\(args, epoch\)', src)
    tool = open(os.path.join(ROOT, 'tools', 'feeder_rate.py')).read()
    assert "'--mosaic'" in tool and 'mosaic=mosaic' in tool
