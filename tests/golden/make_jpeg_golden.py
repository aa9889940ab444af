"""Writes tests/golden/jpeg_golden.npz: a few seeded JPEGs (Pillow-encoded crops of messi.jpg and a noise image, every
supported sampling, grayscale, optimised tables, restart intervals) and Pillow's RGB of each, so that tests/test_jpeg_cpu.py
and tests/test_jpeg_gpu.py pin the decoder's output even where the installed Pillow differs.

    python tests/golden/make_jpeg_golden.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def encode(img, **kw):
    b = io.BytesIO()
    img.save(b, 'JPEG', **kw)
    return b.getvalue()


def main():
    rng = np.random.RandomState(2024)
    messi = Image.open(os.path.join(HERE, 'messi.jpg')).convert('RGB')
    crop = messi.crop((400, 100, 496, 172))          # 96 x 72
    odd = messi.crop((10, 20, 47, 43))               # 37 x 23
    noise = Image.fromarray(rng.randint(0, 256, (24, 40, 3), np.uint8))
    files = [
        encode(crop, quality=75, subsampling=2),
        encode(crop, quality=90, subsampling=1),
        encode(crop, quality=50, subsampling=0),
        encode(odd, quality=75, subsampling=2),
        encode(odd.convert('L'), quality=80),
        encode(crop, quality=75, optimize=True),
        encode(crop, quality=75, restart_marker_blocks=3),
        encode(noise, quality=100),
    ]
    arrays = {}
    for i, f in enumerate(files):
        arrays['jpeg_%d' % i] = np.frombuffer(f, np.uint8)
        arrays['rgb_%d' % i] = np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))
    np.savez_compressed(os.path.join(HERE, 'jpeg_golden.npz'), **arrays)


if __name__ == '__main__':
    main()
