"""The JPEG corpus of tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py: tests/golden/messi.jpg re-encoded by Pillow at test
time over sizes, qualities, subsampling, grayscale, optimised tables and restart intervals, plus noise images at q100 (heavy
in FF00 stuffing).  Seeded: the same bytes on every run of the same Pillow."""
import io
import os

import numpy as np
from PIL import Image

from conftest import ROOT

MESSI = os.path.join(ROOT, 'tests', 'golden', 'messi.jpg')
SIZES = [(1, 1), (2, 8), (3, 8), (4, 17), (1, 17), (7, 5), (17, 33), (100, 75), (640, 480)]     # (widths 1-4: libjpeg replicates
#                                                                  chroma planes of <= 2 columns instead of filtering them)


def encode(img, **kw):
    b = io.BytesIO()
    img.save(b, 'JPEG', **kw)
    return b.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def corpus(sizes=SIZES, seed=0):
    """[(name, bytes)]"""
    rng = np.random.RandomState(seed)
    messi = Image.open(MESSI).convert('RGB')
    out = []
    for size in sizes:
        base = messi.resize(size)
        tag = '%dx%d' % size
        for q in (1, 50, 75, 95, 100):
            for ss in (0, 1, 2):
                out.append(('%s q%d s%d' % (tag, q, ss), encode(base, quality=q, subsampling=ss)))
        out.append(('%s gray' % tag, encode(base.convert('L'), quality=75)))
        out.append(('%s optimize' % tag, encode(base, quality=75, optimize=True)))
        noise = Image.fromarray(rng.randint(0, 256, (size[1], size[0], 3), np.uint8))
        out.append(('%s noise q100' % tag, encode(noise, quality=100)))
        out.append(('%s noise q100 s0' % tag, encode(noise, quality=100, subsampling=0)))
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=4), dict(restart_marker_rows=1)):
            k, v = next(iter(kw.items()))
            out.append(('%s %s=%d' % (tag, k, v), encode(base, quality=75, **kw)))
    out.append(('messi.jpg', open(MESSI, 'rb').read()))
    return out


def voc_like(n, seed=1):
    """n files of about 500x375 at VOC-like qualities, mixed sizes, sampling and restart intervals."""
    rng = np.random.RandomState(seed)
    messi = Image.open(MESSI).convert('RGB')
    out = []
    for i in range(n):
        w, h = int(rng.randint(300, 501)), int(rng.randint(200, 376))
        x0, y0 = int(rng.randint(0, messi.width - w)), int(rng.randint(0, messi.height - h))
        img = messi.crop((x0, y0, x0 + w, y0 + h))
        kw = dict(quality=int(rng.choice([60, 75, 90])), subsampling=int(rng.choice([0, 1, 2, 2])))
        if i % 3 == 1:
            kw['restart_marker_blocks'] = int(rng.choice([1, 4, 16]))
        out.append(('voc %d' % i, encode(img, **kw)))
    return out
