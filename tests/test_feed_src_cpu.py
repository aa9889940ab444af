"""CPU tests of the feeder's by-reference plan (include/yolo355_feed.h: y3f_plan_batch_src): with nothing in the arena it is
y3f_plan_batch's plan byte for byte; with sources in an arena its records are consistent, and the per-pixel functions the
GPU kernels are made of (csrc/y3_feed_px.h, the arena form of window_pixel) run on the host (tests/feed_emul.cpp) give
y3f_sample's bytes.  tests/test_feed_src_gpu.py repeats the comparison with the kernels themselves."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from feed_cases import describe, random_case
from feed_src_cases import POISON, place, ref_jobs


@pytest.fixture(scope='module')
def fn():
    from yolov3_tensorflow_amd import build, feed_native
    build.build_feed(verbose=False)
    return feed_native


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('feed_emul') / 'libfeed_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math',
                           os.path.join(ROOT, 'tests', 'feed_emul.cpp'), '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3f_emulate.restype = ctypes.c_int
    lib.y3f_emulate.argtypes = [ctypes.c_void_p] + [ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.y3f_record_fault.restype = ctypes.c_char_p
    lib.y3f_record_fault.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]
    return lib


def align16(v):
    return (v + 15) // 16 * 16


def test_nothing_in_the_arena_is_the_packed_plan(fn):
    rng = np.random.RandomState(5)
    cases = [random_case(rng, out_size=(48, 48)) for _ in range(64)]
    pjs = [fn.make_job(**c) for c in cases]
    blob, scratch, recs = fn.plan_batch(pjs)
    none = [None] * len(pjs)
    for src1, src2 in ((none, none), (none, None), (None, none)):
        blob_src, scratch_src, recs_src = fn.plan_batch(pjs, src1=src1, src2=src2)
        assert scratch_src == scratch and blob_src.size == blob.size and np.array_equal(blob_src, blob)
        assert bytes(recs_src) == bytes(recs) and all(tuple(d.reserved) == (0, 0, 0) for d in recs_src)
    # sizing only and too small a buffer behave as y3f_plan_batch's
    jobs = fn.job_array(pjs)
    assert fn.plan_sizes(jobs, len(pjs), none, none) == (blob.size, scratch)
    small = np.full(64, 7, np.uint8)
    assert fn.plan_into(jobs, len(pjs), small.ctypes.data, small.size, 0, none, none) == (blob.size, scratch)
    assert (small == 7).all()


def test_records_of_a_mixed_plan_are_consistent(fn):
    rng = np.random.RandomState(5)
    cases = [random_case(rng, out_size=(48, 48)) for _ in range(64)]
    arena, src1, src2 = place(rng, cases)
    assert any(o is None for o in src1) and any(o is not None for o in src1) and any(o is not None for o in src2)
    packed_blob, packed_scratch, packed = fn.plan_batch([fn.make_job(**c) for c in cases])
    blob, scratch, recs = fn.plan_batch(ref_jobs(fn, cases, src1, src2), src1=src1, src2=src2)
    assert scratch == packed_scratch
    saved, end_blob = 0, align16(len(cases) * 208)
    for c, o1, o2, d, p in zip(cases, src1, src2, recs, packed):
        assert d.has2 == (c['img2'] is not None)
        if d.has2:
            assert (o1 is None) != (o2 is None)                 # one member of a pair cached, the other not
        for s, (off, img) in enumerate(((o1, c['img1']), (o2, c['img2']))):
            if img is None:
                continue
            rect = [getattr(d, 'r%d_%s' % (s + 1, f)) for f in ('x0', 'y0', 'w', 'h')]
            assert rect == [getattr(p, 'r%d_%s' % (s + 1, f)) for f in ('x0', 'y0', 'w', 'h')]
            img_off, size = getattr(d, 'img%d_off' % (s + 1)), rect[2] * rect[3] * 3
            if off is None:                                     # packed: inside the blob, behind everything before it
                assert not d.reserved[0] & (1 << s) and d.reserved[1 + s] == 0
                assert img_off % 16 == 0 and img_off >= end_blob and img_off + size <= blob.size
                end_blob = img_off + size
            else:                                               # in the arena: the whole image's offset, stride = its width
                assert d.reserved[0] & (1 << s) and d.reserved[1 + s] == img.shape[1] and img_off == off
                assert rect[0] + rect[2] <= img.shape[1] and rect[1] + rect[3] <= img.shape[0]
                saved += align16(size)
        for name in ('jitter_off', 'xtab_off', 'ytab_off'):     # nothing else moved but by what the sources before it saved
            assert getattr(p, name) - getattr(d, name) == saved
        assert (d.win_off, d.tmp_off) == (p.win_off, p.tmp_off)
    assert saved > 0 and blob.size == packed_blob.size - saved


@pytest.mark.parametrize('interp', range(5))
def test_device_functions_equal_y3f_sample_by_reference(fn, emul, interp):
    rng = np.random.RandomState(300 + interp)
    cases = [random_case(rng, out_size=(48, 48), interp=interp) for _ in range(60)]
    arena, src1, src2 = place(rng, cases)
    blob, scratch_bytes, recs = fn.plan_batch(ref_jobs(fn, cases, src1, src2), src1=src1, src2=src2)
    tables = fn.device_tables()
    for i, d in enumerate(recs):
        assert emul.y3f_record_fault(ctypes.addressof(d), blob.size, arena.size, scratch_bytes) is None, i
    scratch = np.full(max(scratch_bytes, 16), POISON, np.uint8)      # poisoned: nothing may be read before it is written
    out = np.full((len(cases), 48, 48, 3), np.nan, np.float32)
    before = arena.copy()
    assert emul.y3f_emulate(blob.ctypes.data, len(cases), tables.ctypes.data, arena.ctypes.data, scratch.ctypes.data,
                                out.ctypes.data) == 0
    assert np.array_equal(arena, before)
    bad = []
    for i, c in enumerate(cases):
        want = fn.sample(as_float=True, **c)
        if not np.array_equal(out[i], want):
            y, x, ch = np.argwhere(out[i] != want)[0]
            bad.append('%s\n   sources at %r / %r, mode %d, first difference at (y %d, x %d, c %d): %r != %r' %
                       (describe(c), src1[i], src2[i], recs[i].mode, y, x, ch, out[i][y, x, ch] * 255, want[y, x, ch] * 255))
    assert not bad, '%d of %d cases differ:\n%s' % (len(bad), len(cases), '\n'.join(bad[:5]))


def test_record_check_names_what_is_out_of_range(fn, emul):
    """The check y3_feed_run makes before launching (y3fpx::record_fault), on the host: every record of a good plan
    passes at the exact sizes, and fails one byte short of each."""
    rng = np.random.RandomState(11)
    cases = [random_case(rng, out_size=(48, 48)) for _ in range(64)]
    arena, src1, src2 = place(rng, cases, cache_all=True)
    blob, scratch_bytes, recs = fn.plan_batch(ref_jobs(fn, cases, src1, src2), src1=src1, src2=src2)
    fault = lambda d, b=blob.size, a=arena.size, s=scratch_bytes: emul.y3f_record_fault(ctypes.addressof(d), b, a, s)
    seen = set()
    for d in recs:
        assert fault(d) is None
        lw, lh = d.live_x1 - d.live_x0, d.live_y1 - d.live_y0
        if d.r1_w * d.r1_h and not d.has2:
            end = d.img1_off + ((d.r1_y0 + d.r1_h - 1) * d.reserved[1] + d.r1_x0 + d.r1_w) * 3
            assert fault(d, a=end) is None and fault(d, a=end - 1) == b'source rectangle past the arena'
            assert fault(d, a=0) is not None
            keep = d.reserved[1]
            d.reserved[1] = d.r1_x0 + d.r1_w - 1
            assert fault(d) == b"arena row stride smaller than the rectangle's right edge"
            d.reserved[1] = keep
            seen.add('arena')
        if lw * lh:
            assert fault(d, s=d.win_off + lw * lh * 3 - 1) == b'scratch too small'
            keep = d.live_x1
            d.live_x1 = d.win_w + 1
            assert fault(d) == b'live rectangle outside the window'
            d.live_x1 = keep
            seen.add('live')
        if d.colour_on:
            assert fault(d, b=d.jitter_off + 1023) == b'jitter maps past the blob'
        if d.mode in (0, 1, 4) and (d.mode != 4 or d.vertical):
            per = {0: 4, 1: 16, 4: 4 * (2 + d.ksize_y)}[d.mode]
            assert fault(d, b=d.ytab_off + d.res_h * per - 1) is not None      # (the y table is the job's last piece)
            keep = d.ytab_off
            d.ytab_off = blob.size
            assert fault(d) == b'table past the blob'
            d.ytab_off = keep
            seen.add('table')
        assert fault(d) is None
    assert seen == {'arena', 'live', 'table'}


def test_parse_sample_draws_the_same_job_for_a_cached_path_without_opening_it(fn, tmp_path):
    """parse_sample(defer=True, cached=...): for a path the caller holds on the device only (h, w) is needed - same draws,
    same boxes, same job geometry, a NULL source pointer - and the file is not read (it is empty here)."""
    import random
    from PIL import Image
    from yolov3_tensorflow_amd.utils.data_utils import parse_sample
    rng = np.random.RandomState(2)
    lines, sizes = [], {}
    for i, (w, h) in enumerate(((96, 72), (80, 64))):
        path = str(tmp_path / ('img_%d.jpg' % i))
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(path, quality=85)
        sizes[path] = (h, w)
        lines.append('%d %s %d %d 3 10.0 12.0 50.5 40.0 7 30.0 5.0 70.0 60.0' % (i, path, w, h))
    draws = lambda key: dict(rng=np.random.RandomState(key), prng=random.Random(key))
    plain = [parse_sample(line, [64, 64], mode, letterbox, defer=True, **draws(key))
             for key, (line, mode, letterbox) in enumerate(((lines[0], 'train', True), (lines, 'train', False), (lines[1], 'val', True)))]
    for path in sizes:
        open(path, 'wb').close()
    geometry = [name for name, _ in fn.Job._fields_ if name not in ('img1', 'img2', 'colour')]
    for key, (line, mode, letterbox) in enumerate(((lines[0], 'train', True), (lines, 'train', False), (lines[1], 'val', True))):
        idx, pj, boxes, labels = parse_sample(line, [64, 64], mode, letterbox, defer=True, cached=sizes.get, **draws(key))
        want = plain[key]
        assert idx == want[0] and np.array_equal(boxes, want[2]) and np.array_equal(labels, want[3])
        assert all(getattr(pj.job, f) == getattr(want[1].job, f) for f in geometry)
        assert bytes(pj.job.colour) == bytes(want[1].job.colour)
        assert pj.img1 is None and not pj.job.img1 and (pj.key1, pj.key2) == (want[1].key1, want[1].key2)
        assert (pj.img2 is None and not pj.job.img2) and (pj.key2 is not None) == isinstance(line, list)
