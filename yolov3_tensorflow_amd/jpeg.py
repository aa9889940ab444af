# coding: utf-8
"""JPEG decoding on the device, byte-identical to Pillow's `np.asarray(Image.open(f).convert('RGB'))`.

Host (liby3feed.so, include/yolo355_jpeg.h): y3f_jpeg_inspect parses a file's headers; y3f_jpeg_plan turns a batch of
supported files into one relocatable blob (tables, entropy-coded data without stuffing, the chunk cut of the parallel
Huffman decoder) in a recycled pinned buffer, on the library's own threads, without the GIL.  Device (libyolo355.so):
y3_jpeg_decode, three launches on torch's current stream.  Files the device does not decode (progressive, CMYK, 4:1:1,
...) go through Pillow exactly as before, in the same call.
"""
import ctypes
from collections import namedtuple
from ctypes import POINTER, c_int, c_int32, c_int8, c_size_t, c_uint64, c_void_p

import numpy as np

from . import _lib, feed_native
from . import framework as fw

REASONS = {0: "supported", 1: "progressive", 2: "arithmetic coding", 3: "lossless or hierarchical", 4: "not 8-bit",
           5: "colour transform", 6: "sampling factors", 7: "more than one scan", 8: "restart markers", 9: "size"}


class Info(ctypes.Structure):           # y3f_jpeg_info
    _fields_ = [(n, c_int32) for n in ("width", "height", "components", "h_samp", "v_samp", "supported", "reason",
                                        "restart_interval")]


class Rec(ctypes.Structure):            # y3j_rec (272 bytes)
    _fields_ = [(n, c_uint64) for n in ("tables_off", "quant_off", "data_off", "seg_off", "chunk_off", "coef_off",
                                         "plane_off", "state_off", "out_off", "data_bytes")] + \
               [(n, c_int32) for n in ("width", "height", "components", "n_tables", "hmax", "vmax", "mcus_x", "mcus_y",
                                        "blocks_per_mcu", "restart_interval", "n_seg", "n_chunk", "total_blocks")] + \
               [(n, c_int32 * 3) for n in ("comp_bw", "comp_bh", "comp_dw", "comp_dh", "comp_block0", "comp_plane0",
                                            "comp_dc", "comp_ac")] + \
               [("blk_comp", c_int8 * 10), ("blk_dx", c_int8 * 10), ("blk_dy", c_int8 * 10), ("pad", c_int8 * 2),
                ("reserved", c_int32 * 3)]


# name -> (restype, argtypes) of include/yolo355_jpeg.h (liby3feed.so); tests/test_jpeg_cpu.py checks it against the header
PROTOTYPES = {
    "y3f_jpeg_inspect": (c_int, [c_void_p, c_size_t, POINTER(Info)]),
    "y3f_jpeg_plan": (c_int, [POINTER(c_void_p), POINTER(c_size_t), c_int, c_void_p, c_size_t, POINTER(c_size_t),
                              POINTER(c_size_t), POINTER(c_size_t), c_int]),
}

JpegInfo = namedtuple("JpegInfo", "width height components h_samp v_samp supported reason restart_interval")
_bound = None


def _host():
    global _bound
    if _bound is None:
        h = feed_native.lib()
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = restype, argtypes
        _bound = h
    return _bound


def _bytes(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def inspect(data):
    """Headers of one file (bytes) -> JpegInfo; ValueError for a stream that is not a well-formed JPEG."""
    info = Info()
    rc = _host().y3f_jpeg_inspect(data, len(data), ctypes.byref(info))
    if rc != 0:
        raise ValueError("jpeg.inspect: %s" % (_host().y3f_last_error() or b"").decode(errors="replace"))
    return JpegInfo(*(getattr(info, n) for n, _ in Info._fields_))


def _ptrs(datas):
    n = len(datas)
    ptrs = (c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), c_void_p).value for d in datas])
    lens = (c_size_t * n)(*[len(d) for d in datas])
    return ptrs, lens


def plan_sizes(datas, threads=0):
    """(blob bytes, scratch bytes, output bytes) of a batch of supported files."""
    ptrs, lens = _ptrs(datas)
    b, s, o = c_size_t(), c_size_t(), c_size_t()
    feed_native.check(_host().y3f_jpeg_plan(ptrs, lens, len(datas), None, 0, ctypes.byref(b), ctypes.byref(s), ctypes.byref(o),
                                            threads))
    return b.value, s.value, o.value


def plan_into(datas, dst_ptr, capacity, threads=0):
    """Writes the blob at dst_ptr when it fits; returns (blob, scratch, output) bytes (blob > capacity: nothing written)."""
    ptrs, lens = _ptrs(datas)
    b, s, o = c_size_t(), c_size_t(), c_size_t()
    feed_native.check(_host().y3f_jpeg_plan(ptrs, lens, len(datas), dst_ptr, capacity, ctypes.byref(b), ctypes.byref(s),
                                            ctypes.byref(o), threads))
    return b.value, s.value, o.value


def blob_estimate(datas):
    """A blob size that holds a batch of ordinary files (their bytes, the tables, the chunk cut): one planning pass into a
    buffer of this size usually suffices; files with very short restart intervals may need the size the pass reports."""
    return 16 * ((len(datas) * 272 + 15) // 16) + sum(len(d) + len(d) // 4 + 16384 for d in datas)


def _addr(buf):
    return (buf.data_ptr(), buf.numel()) if hasattr(buf, "data_ptr") else (buf.ctypes.data, buf.nbytes)


def plan_blob(datas, take, threads=0):
    """The planning path of decode(): one y3f_jpeg_plan pass into take(blob_estimate) - a second one only when that was
    short.  -> (buffer, blob bytes, scratch bytes, output bytes)."""
    buf = take(blob_estimate(datas))
    need, scratch, out = plan_into(datas, *_addr(buf), threads=threads)
    if need > _addr(buf)[1]:
        buf = take(need)
        need, scratch, out = plan_into(datas, *_addr(buf), threads=threads)
    return buf, need, scratch, out


def plan(datas, threads=0):
    """Host-only: (blob as a uint8 array, scratch bytes, output bytes, [Rec]) - what the tests' emulator runs on."""
    need, scratch, out = plan_sizes(datas, threads)
    blob = np.zeros(max(need, 16), np.uint8)
    got = plan_into(datas, blob.ctypes.data, blob.nbytes, threads)
    assert got == (need, scratch, out)
    n = len(datas)
    recs = [Rec.from_buffer_copy(blob[i * 272:(i + 1) * 272].tobytes()) for i in range(n)]
    return blob, scratch, out, recs


class DecodedBatch(object):
    """The decoded images of one decode() call: a list of uint8 [h, w, 3] device tensors whose status words are checked on
    first access (one host synchronisation on the decode's event, then never again)."""

    def __init__(self, images, status, event, names):
        self._images, self._status, self._event, self._names = images, status, event, names
        self._error = None
        self.rounds = None

    def check(self):
        """Raises ValueError naming the first corrupt file - on every call, not only the first."""
        if self._status is not None:
            self._event.synchronize()
            st = self._status.cpu().numpy().reshape(-1, 2)
            self._status = None
            self.rounds = [int(r) for r in st[:, 1]]
            for (i, name), (code, _) in zip(self._device_items, st):
                if code:
                    self._error = "jpeg.decode: %s is corrupt (device status %d)" % (name, int(code))
                    break
        if self._error is not None:
            raise ValueError(self._error)
        return self

    def __len__(self):
        return len(self._images)

    def __getitem__(self, i):
        self.check()
        return self._images[i]

    def __iter__(self):
        self.check()
        return iter(self._images)


class DeviceJpeg(object):
    """Per device: a pool of pinned blob buffers recycled once their upload has completed (as feed_device.DevicePixels)."""

    def __init__(self, device=None):
        import torch
        self.device = torch.device(device) if device is not None else fw.default_device()
        self.busy = []          # (event, pinned uint8 tensor)

    def _take(self, nbytes):
        import torch
        free = [i for i, (ev, _) in enumerate(self.busy) if ev.query()]
        best = None
        for i in free:
            if self.busy[i][1].numel() >= nbytes and (best is None or self.busy[i][1].numel() < self.busy[best][1].numel()):
                best = i
        if best is not None:
            return self.busy.pop(best)[1]
        for i in reversed(free[:-2]):           # too small for this batch: keep a couple, unpin the rest
            del self.busy[i]
        return torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()

    def decode_supported(self, datas, threads=0):
        """Supported files -> (uint8 device buffer, [Rec], int32 device status [n, 2], event).  Enqueued on torch's current
        stream of the device."""
        import torch
        n = len(datas)
        pinned, need, scratch_bytes, out_bytes = plan_blob(datas, self._take, threads)
        recs = (Rec * n).from_address(pinned.data_ptr())
        recs = [Rec.from_buffer_copy(r) for r in recs]
        with torch.cuda.device(self.device):
            blob = torch.empty(need, dtype=torch.uint8, device=self.device)
            blob.copy_(pinned[:need], non_blocking=True)
            scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=self.device)
            out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=self.device)
            status = torch.empty((n, 2), dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().y3_jpeg_decode(fw.context(self.device), ctypes.c_void_p(blob.data_ptr()), need,
                                                 ctypes.c_void_p(pinned.data_ptr()), n, ctypes.c_void_p(scratch.data_ptr()),
                                                 scratch.numel(), ctypes.c_void_p(out.data_ptr()), out.numel(),
                                                 ctypes.c_void_p(status.data_ptr())))
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        self.busy.append((ev, pinned))
        return out, recs, status, ev

    def decode(self, sources, threads=0):
        import torch
        from PIL import Image
        import io
        datas, names = [], []
        for s in sources:
            datas.append(_bytes(s))
            names.append(s if isinstance(s, str) else "image %d" % len(names))
        sup, images = [], [None] * len(datas)
        for i, d in enumerate(datas):
            try:
                ok = inspect(d).supported
            except ValueError:
                ok = False              # Pillow decodes it - or raises, as it always did
            if ok:
                sup.append(i)
            else:
                images[i] = torch.from_numpy(np.asarray(Image.open(io.BytesIO(d)).convert("RGB")).copy()).to(self.device)
        status, ev = None, None
        if sup:
            out, recs, status, ev = self.decode_supported([datas[i] for i in sup], threads)
            for i, r in zip(sup, recs):
                images[i] = out[r.out_off:r.out_off + 3 * r.width * r.height].view(r.height, r.width, 3)
        batch = DecodedBatch(images, status, ev, names)
        batch._device_items = [(i, names[i]) for i in sup]
        return batch


_decoders = {}


def decode(sources, device=None, threads=0):
    """Files (bytes or paths) -> DecodedBatch: a list of uint8 [h, w, 3] tensors on `device`, Pillow's pixels exactly.
    Raises ValueError naming the file, on first access, if the device found a corrupt stream."""
    import torch
    dev = torch.device(device) if device is not None else fw.default_device()
    dec = _decoders.get(str(dev))
    if dec is None:
        dec = _decoders[str(dev)] = DeviceJpeg(dev)
    return dec.decode(list(sources), threads)
