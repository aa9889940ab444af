"""What the JPEG decoder costs (include/yolo355_jpeg.h), on a corpus generated from a seed and tests/golden/messi.jpg
(VOC-like sizes, about 500x375, qualities 60-90, every supported sampling, a third with restart intervals):

  host      milliseconds per image of what jpeg.decode does on the host (inspect each file, one planning pass, one
            thread) against Pillow's decode of the same files
  device    milliseconds per bs=64 batch of y3_jpeg_decode between device events on the current stream, and the
            synchronisation rounds the entropy decoder took per image (kernel times: run this under
            rocprofv3 --kernel-trace --stats)

    python tools/jpeg_rate.py [--host-only | --device-only] [--batches N]
"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def host(datas):
    from PIL import Image
    from yolov3_tensorflow_amd import jpeg
    best_p = best_j = 1e9
    for _ in range(3):
        t = time.perf_counter()
        for d in datas:
            np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
        best_p = min(best_p, (time.perf_counter() - t) / len(datas))
        t = time.perf_counter()         # what jpeg.decode does on the host: inspect each file, then one planning pass
        for d in datas:
            jpeg.inspect(d)
        jpeg.plan_blob(datas, lambda nbytes: np.empty(nbytes, np.uint8), threads=1)
        best_j = min(best_j, (time.perf_counter() - t) / len(datas))
    print("host: Pillow decode %.3f ms/image, inspect + plan %.3f ms/image (%.1f %%)" % (best_p * 1e3, best_j * 1e3,
                                                                                       100 * best_j / best_p))


def device(datas, batches):
    import ctypes
    import torch
    from yolov3_tensorflow_amd import _lib, jpeg
    from yolov3_tensorflow_amd import framework as fw
    dev = torch.device('cuda:0')
    blob_np, scratch_bytes, out_bytes, recs = jpeg.plan(datas)
    pinned = torch.from_numpy(blob_np).pin_memory()
    blob = pinned.to(dev)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty((len(datas), 2), dtype=torch.int32, device=dev)

    def launch():
        _lib.check(_lib.lib().y3_jpeg_decode(fw.context(dev), ctypes.c_void_p(blob.data_ptr()), blob.numel(),
                                             ctypes.c_void_p(pinned.data_ptr()), len(datas),
                                             ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                                             ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(status.data_ptr())))
    times = []
    for i in range(batches + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if i >= 2:
            times.append(a.elapsed_time(b))
    st = status.cpu().numpy()
    assert (st[:, 0] == 0).all(), st
    rounds = st[:, 1]
    print("device: bs=%d y3_jpeg_decode %.3f ms/batch (median of %d, device events around the three launches)" % (
        len(datas), float(np.median(times)), len(times)))
    print("device: synchronisation rounds per image: min %d median %d max %d" % (rounds.min(), np.median(rounds),
                                                                                   rounds.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--batches', type=int, default=10)
    args = ap.parse_args()
    from jpeg_cases import voc_like
    datas = [d for _, d in voc_like(64)]
    print("corpus: 64 files, %.1f KB mean" % (np.mean([len(d) for d in datas]) / 1024))
    if not args.device_only:
        host(datas)
    if not args.host_only:
        device(datas, args.batches)


if __name__ == '__main__':
    main()
