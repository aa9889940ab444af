"""The JPEG decoder's kernels (y3_jpeg_decode) against Pillow: jpeg.decode gives np.asarray(Image.open(f).convert('RGB'))
byte for byte, over the corpus of tests/jpeg_cases.py, a 64-image mixed batch, messi.jpg, the golden, and a batch whose
progressive members take the Pillow fallback.  Well-formed streams only."""
import os

import numpy as np
import pytest

from conftest import ROOT
from jpeg_cases import MESSI, corpus, encode, pillow_rgb, voc_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def jpeg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from yolov3_tensorflow_amd import jpeg
    return jpeg


def _check(batch, cases):
    assert len(batch) == len(cases)
    for (name, data), img in zip(cases, batch):
        want = pillow_rgb(data)
        assert img.dtype.is_floating_point is False and img.is_cuda
        got = img.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_corpus_is_bit_exact(jpeg):
    cases = corpus()
    batch = jpeg.decode([d for _, d in cases], device='cuda:0')
    _check(batch, cases)
    assert len(batch.rounds) == len(cases) and min(batch.rounds) >= 1


def test_mixed_batch_of_64(jpeg):
    cases = voc_like(64)
    assert any(jpeg.inspect(d).restart_interval for _, d in cases) and any(not jpeg.inspect(d).restart_interval
                                                                            for _, d in cases)
    _check(jpeg.decode([d for _, d in cases], device='cuda:0'), cases)


def test_messi_alone(jpeg):
    batch = jpeg.decode([MESSI], device='cuda:0')
    _check(batch, [('messi.jpg', open(MESSI, 'rb').read())])


def test_golden(jpeg):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_golden.npz'))
    n = len([k for k in g.files if k.startswith('jpeg_')])
    batch = jpeg.decode([g['jpeg_%d' % i].tobytes() for i in range(n)], device='cuda:0')
    for i, img in enumerate(batch):
        assert np.array_equal(img.cpu().numpy(), g['rgb_%d' % i]), i


def test_unsupported_members_take_the_fallback(jpeg):
    from PIL import Image
    base = Image.open(MESSI).convert('RGB')
    cases = [('baseline', encode(base.resize((90, 60)), quality=80)),
             ('progressive', encode(base.resize((70, 50)), quality=80, progressive=True)),
             ('baseline 420 restart', encode(base.resize((64, 64)), quality=70, restart_marker_blocks=2)),
             ('progressive gray', encode(base.resize((33, 17)).convert('L'), quality=90, progressive=True))]
    assert [jpeg.inspect(d).supported for _, d in cases] == [1, 0, 1, 0]
    _check(jpeg.decode([d for _, d in cases], device='cuda:0'), cases)


def test_kernels_read_the_checked_records_not_the_blob(jpeg):
    """y3_jpeg_decode checks recs_host and uploads that copy; the record area at the head of the blob is never read - here
    it is zeroed on the device and the images still come out right."""
    import ctypes
    import torch
    from yolov3_tensorflow_amd import _lib
    from yolov3_tensorflow_amd import framework as fw
    cases = voc_like(4, seed=7) + [('narrow', encode(__import__('PIL.Image').Image.open(MESSI).convert('RGB').resize((3, 9)),
                                                      quality=80, subsampling=2))]
    datas = [d for _, d in cases]
    blob_np, scratch_bytes, out_bytes, recs = jpeg.plan(datas)
    dev = torch.device('cuda:0')
    recs_host = blob_np[:272 * len(datas)].copy()
    blob = torch.from_numpy(blob_np).to(dev)
    blob[:272 * len(datas)] = 0
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    status = torch.full((len(datas), 2), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().y3_jpeg_decode(fw.context(dev), ctypes.c_void_p(blob.data_ptr()), blob.numel(),
                                         ctypes.c_void_p(recs_host.ctypes.data), len(datas),
                                         ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                         ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(status.data_ptr())))
    recs_host[:] = 0            # the call has its own copy: rewriting the caller's records afterwards changes nothing
    torch.cuda.synchronize()
    assert (status[:, 0] == 0).all().item()
    o = out.cpu().numpy()
    for (name, data), r in zip(cases, recs):
        got = o[r.out_off:r.out_off + 3 * r.width * r.height].reshape(r.height, r.width, 3)
        assert np.array_equal(got, pillow_rgb(data)), name
