"""CPU tests of the JPEG decoder (include/yolo355_jpeg.h): the inspector against Pillow, the refusals, and the device
functions (csrc/y3_jpeg_px.h) run on the host in the order the kernels run them (tests/jpeg_emul.cpp) - the same chunks,
the same guessed start states and synchronisation rounds - against np.asarray(Image.open(f).convert('RGB')), bit for bit.
tests/test_jpeg_gpu.py repeats the comparison with the kernels themselves."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT
from jpeg_cases import corpus, encode, pillow_rgb, voc_like

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_golden.npz')
EMUL = os.path.join(ROOT, 'tests', 'jpeg_emul.cpp')


@pytest.fixture(scope='module')
def jpeg():
    from yolov3_tensorflow_amd import build
    build.build_feed(verbose=False)
    from yolov3_tensorflow_amd import jpeg
    return jpeg


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('jpeg_emul') / 'libjpeg_emul.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', EMUL, '-o', out])
    lib = ctypes.CDLL(out)
    lib.y3j_emulate.restype = ctypes.c_int
    lib.y3j_emulate.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def emulate(jpeg, emul, datas):
    """-> ([uint8 HxWx3], status [n, 2])"""
    blob, scratch_bytes, out_bytes, recs = jpeg.plan(datas)
    scratch = np.full(max(scratch_bytes, 16), 0xA5, np.uint8)      # poisoned: the decoder zeroes what it accumulates into
    out = np.zeros(max(out_bytes, 16), np.uint8)
    status = np.full((len(datas), 2), -1, np.int32)
    assert emul.y3j_emulate(blob.ctypes.data, blob.nbytes, len(datas), scratch.ctypes.data, scratch.nbytes,
                            out.ctypes.data, out.nbytes, status.ctypes.data) == 0
    imgs = [out[r.out_off:r.out_off + 3 * r.width * r.height].reshape(r.height, r.width, 3) for r in recs]
    return imgs, status


def test_prototypes_match_the_header(jpeg):
    text = open(os.path.join(ROOT, 'include', 'yolo355_jpeg.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(set(re.findall(r'\b(y3f_[a-z0-9_]+)\s*\(', text))) == sorted(jpeg.PROTOTYPES)
    assert ctypes.sizeof(jpeg.Rec) == 272 and ctypes.sizeof(jpeg.Info) == 32


def test_inspect_matches_pillow(jpeg):
    for name, data in corpus():
        info = jpeg.inspect(data)
        im = Image.open(io.BytesIO(data))
        assert (info.width, info.height) == im.size, name
        assert info.supported == 1 and info.reason == 0, name
        if im.mode == 'L':
            assert info.components == 1, name
        else:
            assert info.components == 3, name
            # Pillow's own reading of the sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
            from PIL import JpegImagePlugin
            ss = JpegImagePlugin.get_sampling(im)
            assert (info.h_samp, info.v_samp) == {0: (1, 1), 1: (2, 1), 2: (2, 2)}[ss], name


def test_unsupported_and_malformed_streams(jpeg):
    base = Image.open(os.path.join(ROOT, 'tests', 'golden', 'messi.jpg')).convert('RGB').resize((64, 48))
    prog = jpeg.inspect(encode(base, quality=75, progressive=True))
    assert prog.supported == 0 and jpeg.REASONS[prog.reason] == 'progressive' and (prog.width, prog.height) == (64, 48)
    cmyk = jpeg.inspect(encode(base.convert('CMYK'), quality=75))
    assert cmyk.supported == 0 and cmyk.components == 4 and jpeg.REASONS[cmyk.reason] == 'colour transform'
    good = encode(base, quality=75)
    for cut in (2, 20, len(good) // 2, len(good) - 2, len(good) - 1):
        with pytest.raises(ValueError):
            jpeg.inspect(good[:cut])
    with pytest.raises(ValueError):
        jpeg.inspect(b'not a jpeg at all')
    # a missing Huffman table: drop every DHT segment
    i, stripped = 2, bytearray(good[:2])
    while good[i + 1] != 0xDA:
        n = 2 + (good[i + 2] << 8 | good[i + 3])
        if good[i + 1] != 0xC4:
            stripped += good[i:i + n]
        i += n
    stripped += good[i:]
    with pytest.raises(ValueError, match='Huffman'):
        jpeg.inspect(bytes(stripped))
    # the planner refuses what the inspector reports unsupported
    with pytest.raises(RuntimeError, match='image 1'):
        jpeg.plan([good, encode(base, quality=75, progressive=True)])


def test_emulated_decode_is_bit_exact_over_the_corpus(jpeg, emul):
    cases = corpus()
    imgs, status = emulate(jpeg, emul, [d for _, d in cases])
    rounds = {}
    for (name, data), img, (st, r) in zip(cases, imgs, status):
        assert st == 0, name
        want = pillow_rgb(data)
        assert img.shape == want.shape and np.array_equal(img, want), name
        rounds[name] = int(r)
    assert all(r >= 1 for r in rounds.values())


def test_emulated_decode_of_a_mixed_batch(jpeg, emul):
    cases = voc_like(12)
    imgs, status = emulate(jpeg, emul, [d for _, d in cases])
    assert (status[:, 0] == 0).all()
    for (name, data), img in zip(cases, imgs):
        assert np.array_equal(img, pillow_rgb(data)), name


def test_golden(jpeg, emul):
    g = np.load(GOLDEN)
    n = len([k for k in g.files if k.startswith('jpeg_')])
    datas = [g['jpeg_%d' % i].tobytes() for i in range(n)]
    imgs, status = emulate(jpeg, emul, datas)
    assert (status[:, 0] == 0).all()
    for i, img in enumerate(imgs):
        assert np.array_equal(img, g['rgb_%d' % i]), i


def _corrupted(seed=3):
    """(name, bytes, must_fail): streams with their scan cut off (must fail) or bytes of the scan changed (may decode)."""
    rng = np.random.RandomState(seed)
    base = Image.open(os.path.join(ROOT, 'tests', 'golden', 'messi.jpg')).convert('RGB').resize((120, 88))
    out = []
    for ss in (0, 1, 2):
        good = encode(base, quality=85, subsampling=ss)
        sos = good.index(b'\xff\xda')
        start = sos + 2 + (good[sos + 2] << 8 | good[sos + 3])
        end = len(good) - 2
        for frac in (0.1, 0.5, 0.9):
            cut = start + int((end - start) * frac)
            body = good[:cut].rstrip(b'\xff')
            out.append(('cut %d %.1f' % (ss, frac), body + b'\xff\xd9', True))
        for k in range(4):
            b = bytearray(good)
            for _ in range(1 + k * 4):
                p = int(rng.randint(start, end))
                b[p] = int(rng.randint(0, 255))         # (never 0xFF: no new markers)
                if b[p - 1] == 0xFF:
                    b[p] = 0
            out.append(('flip %d %d' % (ss, k), bytes(b), False))
        # a run of all-ones codes: no table has them
        b = bytearray(good)
        for p in range(start + (end - start) // 3, start + (end - start) // 3 + 16, 2):
            b[p], b[p + 1] = 0xFF, 0x00
        out.append(('ones %d' % ss, bytes(b), True))
    return out


def test_corrupt_streams_set_a_bad_status(jpeg, emul):
    cases = [c for c in _corrupted() if jpeg.inspect(c[1]).supported]
    assert sum(1 for c in cases if c[2]) >= 9
    imgs, status = emulate(jpeg, emul, [d for _, d, _ in cases])
    for (name, _, must_fail), (st, _) in zip(cases, status):
        if must_fail:
            assert st != 0, name


def test_corrupt_streams_under_address_sanitizer(jpeg, tmp_path):
    """The emulator built with -fsanitize=address, every buffer exactly as large as the plan says: no read or write past
    an extent, whatever the stream holds."""
    exe = str(tmp_path / 'jpeg_emul_asan')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-omit-frame-pointer',
                           '-DY3J_EMUL_MAIN', EMUL, '-o', exe])
    cases = [c for c in _corrupted() if jpeg.inspect(c[1]).supported]
    datas = [d for _, d, _ in cases] + [d for _, d in voc_like(3)]
    blob, scratch_bytes, out_bytes, _ = jpeg.plan(datas)
    path = str(tmp_path / 'blob.bin')
    blob[:jpeg.plan_sizes(datas)[0]].tofile(path)
    res = subprocess.run([exe, path, str(len(datas)), str(scratch_bytes), str(out_bytes)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0',
                                                          UBSAN_OPTIONS='halt_on_error=1'))
    assert res.returncode == 0, res.stderr.decode(errors='replace')[-3000:]
    st = [int(v) for v in res.stdout.split()]
    assert len(st) == len(datas)
    for (name, _, must_fail), s in zip(cases, st):
        if must_fail:
            assert s != 0, name
    assert st[len(cases):] == [0, 0, 0]


def test_a_corrupt_status_raises_on_every_access():
    import torch
    from yolov3_tensorflow_amd import jpeg

    class Done(object):
        def synchronize(self):
            pass

    imgs = [torch.zeros((2, 2, 3), dtype=torch.uint8), torch.zeros((1, 1, 3), dtype=torch.uint8)]
    batch = jpeg.DecodedBatch(imgs, torch.tensor([[0, 2], [4, 9]], dtype=torch.int32), Done(), ['a.jpg', 'b.jpg'])
    batch._device_items = [(0, 'a.jpg'), (1, 'b.jpg')]
    for _ in range(3):
        with pytest.raises(ValueError, match='b.jpg'):
            batch[0]
        with pytest.raises(ValueError, match='b.jpg'):
            list(batch)
    assert batch.rounds == [2, 9]


def test_narrow_subsampled_planes_are_replicated(jpeg, emul):
    """libjpeg filters a chroma plane only when it is more than 2 samples wide; narrower ones are replicated."""
    base = Image.open(os.path.join(ROOT, 'tests', 'golden', 'messi.jpg')).convert('RGB')
    cases = [(w, h, ss) for w in range(1, 7) for h in (1, 2, 3, 8, 17) for ss in (1, 2)]
    datas = [encode(base.resize((w, h)), quality=75, subsampling=ss) for w, h, ss in cases]
    imgs, status = emulate(jpeg, emul, datas)
    assert (status[:, 0] == 0).all()
    for c, d, img in zip(cases, datas, imgs):
        assert np.array_equal(img, pillow_rgb(d)), c
