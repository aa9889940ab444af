# coding: utf-8
"""The training / validation feeder (reference train.py:34-52 + utils/data_utils.py:179-224):

    tf.data.TextLineDataset -> shuffle -> batch -> map(py_func(get_batch_data), num_parallel_calls=10) -> prefetch(5)

rebuilt for one process per GPU with the device-resident target assignment of this package:

  * `num_threads` workers (reference: args.num_threads = 10) decode, augment and resize ONE image each
    (utils.data_utils.parse_sample).  The pixel work - blend, colour jitter, crop, resize, pad, flip, /255 - and the crop
    search run in liby3feed.so (include/yolo355_feed.h: native code where the reference's is OpenCV), which releases the
    GIL, as PIL's JPEG decoder does; a worker holds the GIL for a little under a millisecond per image (which levels one
    process off at 1,000-1,200 images/s: profiles/r03_feeder_rate.txt).  So the workers are THREADS by default
    (backend='thread'); backend='process' scales past one interpreter's GIL (3,320 images/s with 32 workers) and is the
    default for the numpy / Pillow pixel path (Y3_FEED_NATIVE=0), which holds the GIL most of the time.  The processes come
    from a `forkserver` (one pool per process and worker count, shared by the training and the validation feeder): forking
    the training process itself copies every PINNED host page eagerly - measured 93 s for four workers once 8 GB were
    pinned, against 0.4 s in a fresh process (tools/feeder_diag.py) - and the feeder is what pins them.  (As with any start
    method but fork, a SCRIPT that builds a process-backed Feeder needs the usual `if __name__ == '__main__':` guard.)
  * how a batch comes back from the workers is a DELIVERY, chosen once per epoch (Feeder._delivery) and told in its class:
    _HostPixels (threads write float32 slots of a pinned batch buffer: no pickling, no second pass), _DeferredPixels
    (pixels='gpu'), _SharedPixels (processes; without /dev/shm it falls back to _HostPixels' pickled 8-bit images);
  * the host half, Feeder._host_batches, keeps `prefetch` batches of jobs in flight and yields them collated, oldest first.
    It touches no device (tools/feeder_rate.py --host-only and the tests run it alone, over numpy buffers);
  * the device half, Feeder.epoch: a coordinator thread copies each host batch to the device on a SIDE stream; a bounded
    queue of `prefetch` batches (reference: prefetech_buffer = 5) decouples it from the train step, so decode / resize /
    H2D of batch i+1.. overlap the step on batch i.  The pinned buffers are recycled once their copy has completed
    (_Buffers: pinning 130 MB per batch afresh costs more than filling it);
  * pixels='gpu': the workers only decode and draw (parse_sample(defer=True)); the coordinator plans the batch's pixel
    work (liby3feed.so: y3f_plan_batch, native threads), uploads ONE blob of 8-bit sources and tables and runs y3_feed_run
    on the side stream (feed_device.DevicePixels) - the same bytes as the host path, 5 of the 5.9 ms a core spends per
    image moved to three launches of a few hundred microseconds per batch;
  * cache_bytes > 0 (with pixels='gpu'): every file is decoded once; its 8-bit pixels stay in a device arena of that many
    bytes (feed_cache.SourceCache, kept over the epochs, nothing evicted) and later uses read them there by reference
    (y3f_plan_batch_src / y3_feed_run): no decode, no source bytes in the blob.  The same batches, byte for byte;
  * the consumer makes its compute stream wait for the copy's event (no host synchronisation) and runs `y3_process_box`
    for the whole batch on the device (utils.data_utils.process_box_batch: bit-exact against the reference's
    process_box), so the three y_true tensors (3.6 MB per 416x416 image - more than the image itself) never cross PCIe;
  * multi-scale: a new size every `interval` batches, drawn exactly like get_batch_data (random.seed(count // interval)
    over range(10, 20) * 32 = 320 .. 608); mix-up pairing per batch; every random draw comes from generators seeded by
    (seed, epoch, batch, sample), so a run is reproducible whatever the thread interleaving (the reference's is not);
  * data parallel: rank r of `world` takes samples r::world of every global batch (same shuffle on every rank);
  * mosaic=True ('train' only): every image of a batch is cut together from four samples - the batch's own entry and three
    lines drawn from the whole file (utils.data_utils.mosaic_lines; grouped before the rank split).  The 4 * n samples go
    through the chain above unchanged, by whichever delivery is configured; the coordinator then composes them on the side
    stream (utils.data_utils.mosaic_batch -> y3_mosaic: windows copied, boxes clipped, filtered and compacted; the rule is
    in include/yolo355.h) and the consumer assigns targets to the composed [n][4 * kmax][5] boxes.  Four samples' cost per
    image, and 4 * n images of staging memory per batch in flight.  `feeder.mosaic` is read once per epoch;
  * affine=(degrees, translate, scale, shear) ('train' only): every delivered image, composed or not, is warped by its own
    random rotation / zoom / shear / translation on the side stream (utils.data_utils.affine_batch -> y3_affine: bilinear
    resampling through a Q16 inverse map, the letterbox grey outside; boxes mapped, clipped, filtered and compacted; the rule
    is in include/yolo355.h), behind the composition when mosaic is on.  The host adds six draws and a 3 x 3 product per
    image (utils.data_aug.affine_draw, _affine_records).  `feeder.affine` is read once per epoch.
"""
from __future__ import division, print_function

import queue
import random
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from itertools import islice

import numpy as np


def _worker_sample(job, out=None, defer=False, cached=None):
    """One sample in a worker: job = (line or mix-up pair, [w, h], mode, letterbox, rng key).  A thread is handed `out`, its
    float32 slot of the batch buffer; a process returns the 8-bit image (a quarter of the bytes to pickle); `defer`: the
    decoded sources and the pixel JOB come back, the pixels are left to the device; `cached`: path -> (h, w) of a source
    the feeder's cache holds (it is not decoded again) or None."""
    from .utils.data_utils import parse_sample
    line, size, mode, letterbox, key = job
    return parse_sample(line, size, mode, letterbox, rng=np.random.RandomState(key % (2 ** 31)), prng=random.Random(key),
                        as_uint8=out is None and not defer, out=out, defer=defer, cached=cached)


_ATTACHED = {}        # (in a worker process) path of a shared batch buffer -> its mapping


def _worker_sample_shared(job, path, shape, index):
    """One sample in a worker PROCESS, written as float32 straight into slot `index` of the batch buffer the parent keeps in
    shared memory at `path` ([n, h, w, 3]); only the boxes and labels travel back through the pipe."""
    arr = _ATTACHED.get(path)
    if arr is None:
        if len(_ATTACHED) >= 32:            # the parent recycles a handful of buffers; anything older is gone
            _ATTACHED.clear()
        arr = _ATTACHED[path] = np.memmap(path, dtype=np.float32, mode='r+', shape=tuple(shape))
    idx, _, boxes, labels = _worker_sample(job, out=arr[index])
    return idx, None, boxes, labels


class _Buffers(object):
    """Batch buffers by shape, handed out again once the H2D copy that read them has completed.  A subclass says what a
    buffer is (`_make`, `_shape`) and how it goes (`_drop`); as it stands: plain numpy arrays, for a host half run alone."""

    def __init__(self):
        self.busy = []          # (event, buffer)

    def take(self, shape):
        shape = tuple(int(v) for v in shape)
        free = [i for i, (ev, _) in enumerate(self.busy) if ev is None or ev.query()]
        for i in free:
            if self._shape(self.busy[i][1]) == shape:
                return self.busy.pop(i)[1]
        # none of this shape is free.  Multi-scale training moves from size to size: keep a handful of free buffers of
        # other shapes (the size may come back), let go of the rest
        for i in reversed(free[:-4]):
            self._drop(self.busy.pop(i)[1])
        return self._make(shape)

    def give(self, event, buf):
        self.busy.append((event, buf))      # free again once `event` has completed (None: nothing reads it any more)

    def _make(self, shape):
        return np.empty(shape, np.float32)

    def _shape(self, buf):
        return tuple(buf.shape)

    def _drop(self, buf):
        pass


class _PinnedBuffers(_Buffers):       # (tensors)
    def _make(self, shape):
        import torch
        return torch.empty(shape, dtype=torch.float32).pin_memory()


class _SharedBuffers(_Buffers):
    """Batch buffers for worker processes: files in /dev/shm mapped here and in the workers, page-locked for the device
    (hipHostRegister) so that the upload reads them like any pinned buffer.  Where shared memory or the registration is not
    available, `take` returns None and the feeder falls back to pickled 8-bit images."""

    _live = []              # instances with files in /dev/shm: closed at interpreter exit at the latest

    def __init__(self):
        _Buffers.__init__(self)
        self.entries = []       # every live entry: dict(path, map, array, tensor, registered)
        self.broken = False
        if not _SharedBuffers._live:
            import atexit
            atexit.register(_SharedBuffers._close_all)
        _SharedBuffers._live.append(self)

    @staticmethod
    def _close_all():
        for inst in list(_SharedBuffers._live):
            inst.close()

    def _make(self, shape):
        import mmap
        import os
        import tempfile
        import torch
        nbytes = int(np.prod(shape)) * 4
        fd, path = tempfile.mkstemp(prefix='y3feed_%d_' % os.getpid(), dir='/dev/shm')
        try:
            os.ftruncate(fd, nbytes)
            mapping = mmap.mmap(fd, nbytes)
        finally:
            os.close(fd)
        array = np.frombuffer(mapping, np.float32).reshape(shape)
        tensor = torch.from_numpy(array)
        registered = False
        have_device = torch.cuda.is_available()
        if have_device:
            try:
                registered = int(torch.cuda.cudart().cudaHostRegister(tensor.data_ptr(), nbytes, 0)) == 0
            except Exception:       # noqa: BLE001 - no such entry point
                registered = False
        if have_device and not registered:
            # The raw return code leaves HIP's per-thread last-error set (memlock ulimit, an unsupported /dev/shm mapping):
            # clear it, or the next launch check of PyTorch on this thread reports an unrelated "HIP error".  And stop
            # using shared buffers: an unpinned mapping would mean synchronous pageable copies - the pickled 8-bit path
            # (take() -> None) is the better fallback.
            try:
                import ctypes
                ctypes.CDLL('libamdhip64.so').hipGetLastError()
            except OSError:
                pass
            self.broken = True
        entry = dict(path=path, map=mapping, array=array, tensor=tensor, registered=registered)
        self.entries.append(entry)
        return entry

    def _shape(self, entry):
        return tuple(entry['array'].shape)

    def take(self, shape):
        if self.broken:
            return None
        try:
            entry = _Buffers.take(self, shape)
        except (OSError, ValueError):
            self.broken = True
            return None
        if self.broken:                 # (the mapping could not be page-locked)
            self._drop(entry)
            return None
        return entry

    def _drop(self, entry):
        import os
        import torch
        if entry in self.entries:
            self.entries.remove(entry)
        try:
            if entry['registered']:
                torch.cuda.cudart().cudaHostUnregister(entry['tensor'].data_ptr())
        except Exception:       # noqa: BLE001
            pass
        entry['tensor'] = entry['array'] = None
        try:
            entry['map'].close()
        except (BufferError, ValueError):       # a view is still alive somewhere: the mapping goes with it
            pass
        try:
            os.unlink(entry['path'])
        except OSError:
            pass

    def close(self):
        self.busy = []
        for entry in list(self.entries):
            self._drop(entry)
        if self in _SharedBuffers._live:
            _SharedBuffers._live.remove(self)


_POOLS = {}
_POOLS_LOCK = threading.Lock()


def _shared_process_pool(workers):
    import atexit
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    with _POOLS_LOCK:
        pool = _POOLS.get(workers)
        if pool is None:
            ctx = multiprocessing.get_context('forkserver')
            ctx.set_forkserver_preload(['yolov3_tensorflow_amd.utils.data_utils', 'yolov3_tensorflow_amd.utils.data_aug'])
            pool = _POOLS[workers] = ProcessPoolExecutor(workers, mp_context=ctx)
            if len(_POOLS) == 1:
                atexit.register(_shutdown_pools)
        return pool


def _shutdown_pools():
    with _POOLS_LOCK:
        for pool in _POOLS.values():
            pool.shutdown(wait=False, cancel_futures=True)
        _POOLS.clear()


class _DeferredPixels(object):
    """Delivery with pixels='gpu': worker threads decode and draw; the batch comes back as pixel JOBS for the device.
    Every delivery has two steps.  `submit(pool, jobs, shape)` takes the batch buffer it needs, submits the worker calls and
    returns `pending` = (futures, owner, buffer); `collect(pending)` waits for them and returns the collated host batch:
    (ids, images or pixel jobs, boxes, labels, counts, owner).  owner = (pool of buffers, buffer) to hand back, or None."""

    def __init__(self, cached):
        self.cached = cached        # path -> (h, w) of a source the feeder's cache holds, or None

    def submit(self, pool, jobs, shape):
        return [pool.submit(_worker_sample, job, None, True, self.cached) for job in jobs], None, None

    def collect(self, pending):
        from .utils.data_utils import collate
        samples = [f.result() for f in pending[0]]
        ids, _, boxes, labels, counts = collate(samples, with_images=False)
        return ids, [s[1] for s in samples], boxes, labels, counts, None


class _HostPixels(object):
    """Delivery of float32 images in a batch buffer of `buffers`: worker threads write their slots of it (in_place), or
    worker processes hand back 8-bit images (a quarter of the bytes to pickle) that `collect` divides into it."""

    def __init__(self, buffers, in_place):
        self.buffers, self.in_place = buffers, in_place

    def submit(self, pool, jobs, shape):
        buf = self.buffers.take(shape)
        slots = np.asarray(buf) if self.in_place else [None] * len(jobs)
        return [pool.submit(_worker_sample, job, slots[j]) for j, job in enumerate(jobs)], (self.buffers, buf), buf

    def collect(self, pending):
        from .utils.data_utils import collate
        futs, owner, buf = pending
        slots = np.asarray(buf)         # (a view of the tensor's memory)
        samples = [f.result() for f in futs]
        samples = [(s[0], slots[j] if s[1] is None else s[1], s[2], s[3]) for j, s in enumerate(samples)]
        ids, _, boxes, labels, counts = collate(samples, out_images=slots)
        return ids, buf, boxes, labels, counts, owner


class _SharedPixels(_HostPixels):
    """Delivery by worker processes that fill a shared, page-locked batch buffer of `shared`; a batch for which there is
    none (no /dev/shm, no registration: then for every later batch too) travels as pickled 8-bit images."""

    def __init__(self, shared, buffers):
        _HostPixels.__init__(self, buffers, False)
        self.shared = shared

    def submit(self, pool, jobs, shape):
        entry = self.shared.take(shape)
        if entry is None:
            return _HostPixels.submit(self, pool, jobs, shape)
        futs = [pool.submit(_worker_sample_shared, job, entry['path'], shape, j) for j, job in enumerate(jobs)]
        return futs, (self.shared, entry), entry['tensor']


class Batch(object):
    """image_ids (list), images [n,h,w,3] float32 device tensor, y_true (three device tensors), img_size [w, h]."""
    __slots__ = ('image_ids', 'images', 'y_true', 'img_size', 'boxes', 'labels', 'counts')


class Feeder(object):
    def __init__(self, lines, batch_size, class_num, img_size, anchors, mode='train', multi_scale=False, use_mix_up=False,
                 letterbox_resize=True, num_threads=10, prefetch=5, shuffle=None, seed=0, rank=0, world=1, interval=10,
                 device=None, drop_remainder=False, backend=None, pixels=None, cache_bytes=0, mosaic=False,
                 mosaic_min_side=2.0, mosaic_min_visible=0.25, affine=None, affine_min_side=2.0, affine_min_area=0.1,
                 affine_max_aspect=20.0, assign_iou_thresh=1.0):
        from .utils.data_utils import _check_assign_iou_thresh
        # below 1: every anchor whose shape IoU with a box exceeds it is a positive too (utils.data_utils.process_box_host)
        self.assign_iou_thresh = _check_assign_iou_thresh(assign_iou_thresh)
        self.lines =[l for l in lines if (l.strip() if isinstance(l, str) else l)]
        self.batch_size, self.class_num = int(batch_size), int(class_num)
        self.img_size, self.anchors = list(img_size), np.asarray(anchors, np.float32).reshape(9, 2)
        self.mode = mode
        self.multi_scale = bool(multi_scale) and mode == 'train'
        self.use_mix_up = bool(use_mix_up) and mode == 'train'
        self.letterbox = bool(letterbox_resize)
        self.num_threads, self.prefetch = max(1, int(num_threads)), max(1, int(prefetch))
        self.shuffle = (mode == 'train') if shuffle is None else bool(shuffle)
        self.seed, self.rank, self.world, self.interval = int(seed), int(rank), int(world), int(interval)
        self.device = device
        self.drop_remainder = drop_remainder
        self.batches_served = 0          # the reference's iter_cnt: counts batches over epochs (multi-scale schedule)
        if backend is None:      # threads when the pixel work is native code that releases the GIL (module docstring)
            from . import feed_native
            backend = 'thread' if feed_native.enabled() else 'process'
        if backend not in ('process', 'thread'):
            raise ValueError("backend must be 'process' or 'thread'")
        self.backend = backend
        if pixels is None:      # on the device wherever the workers can hand decoded sources over (same bytes either way)
            from . import feed_native
            pixels = 'gpu' if backend == 'thread' and feed_native.enabled() else 'host'
        if pixels not in ('host', 'gpu'):
            raise ValueError("pixels must be 'host' or 'gpu'")
        if pixels == 'gpu':
            from . import feed_native
            if backend != 'thread' or not feed_native.enabled():
                raise ValueError("pixels='gpu' runs with the thread backend and the native job builder (Y3_FEED_NATIVE=1): "
                                 "the workers hand decoded sources to the coordinator")
        self.pixels = pixels
        self.cache_bytes = int(cache_bytes)
        if self.cache_bytes < 0 or (self.cache_bytes > 0 and pixels != 'gpu'):
            raise ValueError("cache_bytes > 0 keeps decoded sources on the device for the device's pixel work: it needs "
                             "pixels='gpu' (thread backend, native job builder)")
        if mosaic and mode != 'train':
            raise ValueError("mosaic=True composes augmented training samples: it needs mode='train'")
        self.mosaic = bool(mosaic)  # read once per epoch: a caller may switch it off between epochs ("close mosaic")
        self.mosaic_min_side, self.mosaic_min_visible = float(mosaic_min_side), float(mosaic_min_visible)
        if affine is not None:
            if mode != 'train':
                raise ValueError("affine=(degrees, translate, scale, shear) warps augmented training samples: it needs "
                                 "mode='train'")
            affine = tuple(float(v) for v in affine)
            if len(affine) != 4:
                raise ValueError("affine must be None or (degrees, translate, scale, shear)")
        self.affine = affine        # read once per epoch: a caller may set it to None between epochs
        self.affine_min_side, self.affine_min_area = float(affine_min_side), float(affine_min_area)
        self.affine_max_aspect = float(affine_max_aspect)
        self.cache = None           # feed_cache.SourceCache, made with the side stream's device; lives as long as the feeder
        self._pool = None
        self._side = None           # (device, side stream, DevicePixels or None)

    def _executor(self):
        """The worker pool: one per process and worker count, created on first use and shared by every Feeder (see the
        module docstring for why the workers are not forked from this process)."""
        if self.backend == 'thread':
            if self._pool is None:
                self._pool = ThreadPoolExecutor(self.num_threads)
            return self._pool
        return _shared_process_pool(self.num_threads)

    def close(self):
        if self._pool is not None:          # (only thread pools are owned by the feeder)
            self._pool.shutdown(wait=False, cancel_futures=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 - interpreter shutdown
            pass

    def __len__(self):
        n = len(self.lines)
        return n // self.batch_size if self.drop_remainder else (n + self.batch_size - 1) // self.batch_size

    # ---- host side ------------------------------------------------------------------------------------------------
    def _plan(self, epoch):
        """[(batch number within the epoch, img_size, [line or mix-up pair, ...] of THIS rank)] for one epoch.  With mosaic on,
        an entry is (batch number, img_size, [group of four lines or mix-up pairs, ...], [record, ...], [own, ...]) of this
        rank: utils.data_utils.mosaic_lines' groups, formed before the rank split, one utils.data_aug.mosaic_draw record per
        image, and the position of the batch's own entry in its group."""
        mosaic = self.mosaic and self.mode == 'train'
        order = list(range(len(self.lines)))
        if self.shuffle:
            random.Random(self.seed * 1000003 + epoch).shuffle(order)      # same order on every rank
        plan = []
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            size = list(self.img_size)
            if self.multi_scale:
                from .utils.data_utils import multi_scale_size
                size = multi_scale_size(self.batches_served + b, self.interval)
            lines = [self.lines[i] for i in idx]
            if self.use_mix_up:
                from .utils.data_utils import mix_up_lines
                key = (self.seed * 1000003 + epoch) * 100003 + b
                lines = mix_up_lines(lines, rng=np.random.RandomState(key % (2 ** 31)), prng=random.Random(key))
            if mosaic:
                from .utils.data_aug import mosaic_draw
                from .utils.data_utils import mosaic_lines
                key = (self.seed * 1000003 + epoch) * 100003 + b
                groups, own = mosaic_lines(lines, self.lines, random.Random('mosaic-groups-%d' % key))
                records = [mosaic_draw(random.Random('mosaic-record-%d-%d' % (key, slot)), size[0], size[1])
                           for slot in range(len(groups))]
                mine = slice(self.rank, None, self.world) if groups[self.rank::self.world] else slice(0, 1)
                plan.append((b, size, groups[mine], records[mine], own[mine]))
                continue
            mine = lines[self.rank::self.world] or lines[:1]
            plan.append((b, size, mine))
        return plan

    def _affine_records(self, epoch, entry, affine):
        """One utils.data_aug.affine_draw record per delivered image of one entry of the plan, for the ranges `affine`.  Image
        j of this rank is slot rank + j * world of the global batch, and the record is drawn from (key, slot) as the mosaic
        records are: it depends on neither the workers, the backend nor the number of ranks."""
        from .utils.data_aug import affine_draw
        b, size, lines = entry[:3]
        key = (self.seed * 1000003 + epoch) * 100003 + b
        whole = min(self.batch_size, len(self.lines) - b * self.batch_size)
        first = self.rank if self.rank < whole else 0       # (a rank with no share of a short batch takes slot 0, as in _plan)
        return [affine_draw(random.Random('affine-record-%d-%d' % (key, first + j * self.world)), size[0], size[1], *affine)
                for j in range(len(lines))]

    def _job(self, epoch, b, j, line, size, tile=None):
        key = ((self.seed * 1000003 + epoch) * 100003 + b) * 1009 + j * self.world + self.rank
        if tile is not None:        # sample `tile` of mosaic image j
            key = key * 4 + tile
        return (line, size, self.mode, self.letterbox, key)

    def _jobs(self, epoch, entry):
        """The worker jobs of one entry of the plan, in sample order: n of them, or 4 * n (sample 4 * j + tile) with mosaic."""
        b, size, lines = entry[:3]
        if len(entry) == 3:
            return [self._job(epoch, b, j, line, size) for j, line in enumerate(lines)]
        return [self._job(epoch, b, j, line, size, tile) for j, group in enumerate(lines) for tile, line in enumerate(group)]

    def _delivery(self, buffers, shared, cached=None):
        """How this feeder's batches come from the workers (module docstring), over the given pools of batch buffers."""
        if self.pixels == 'gpu':
            return _DeferredPixels(cached)
        if self.backend == 'thread':
            return _HostPixels(buffers, True)
        return _SharedPixels(shared, buffers)

    def _host_batches(self, epoch, delivery, stop, plan=None):
        """The host half of an epoch, which needs no device: keeps up to `prefetch` batches of worker jobs in flight and
        yields (img_size,) + delivery.collect(oldest) until the plan is served or `stop` is set.  The consumer hands each
        batch's buffer back (owner[0].give); the buffers of batches never collected are let go here.  plan: _plan(epoch) where
        the caller has made it already.  A mosaic entry is delivered as its 4 * n samples; composing them is the device half's."""
        pool = self._executor()
        pending = []
        plan = iter(self._plan(epoch) if plan is None else plan)
        try:
            while not stop.is_set():
                for entry in islice(plan, self.prefetch - len(pending)):
                    size, jobs = entry[1], self._jobs(epoch, entry)
                    pending.append((size, delivery.submit(pool, jobs, (len(jobs), size[1], size[0], 3))))
                if not pending:
                    break
                size, oldest = pending.pop(0)
                yield (size,) + delivery.collect(oldest)
        finally:
            for _, (_, owner, _) in pending:        # (workers may still be writing: dropped, never handed out again)
                if owner is not None:
                    owner[0]._drop(owner[1])

    def epoch(self, epoch=0):
        """Iterate over one epoch: yields Batch objects whose tensors live on the device.  The device half: a coordinator
        thread uploads what _host_batches delivers on a side stream, the consumer assigns the targets."""
        import torch
        from . import framework as fw
        from .utils.data_utils import affine_batch, mosaic_batch, pad_fill, process_box_batch
        dev = torch.device(self.device) if self.device is not None else fw.default_device()
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        # one side stream (and, with pixels='gpu', one set of device tables + pinned blob buffers) per feeder and device, kept
        # over the epochs: framework.context() caches a y3_ctx per (device, stream)
        if self._side is None or self._side[0] != dev:
            self._side = (dev, torch.cuda.Stream(device=dev), None)
        copy_stream = self._side[1]

        on_device = self.pixels == 'gpu'
        device_pixels = None
        if on_device:
            if self._side[2] is None:
                from .feed_device import DevicePixels
                self._side = (dev, copy_stream, DevicePixels(dev))
            device_pixels = self._side[2]
            if self.cache_bytes > 0 and (self.cache is None or self.cache.device != dev):
                from .feed_cache import SourceCache
                self.cache = SourceCache(dev, self.cache_bytes)
        cache = self.cache if on_device and self.cache_bytes > 0 else None
        shared = _SharedBuffers()       # (no file in /dev/shm before a worker process needs one)
        delivery = self._delivery(_PinnedBuffers(), shared, cache.shape_of if cache is not None else None)

        def put(item):
            # every hand-over gives up as soon as the consumer has stopped: a blocking put on a full queue that nobody
            # drains any more would park this thread - and the device tensors / pinned buffers it holds - for good
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return
                except queue.Full:
                    continue

        plan = self._plan(epoch)        # (reads self.mosaic: once per epoch)
        affine = self.affine if self.mode == 'train' else None      # (likewise)

        def produce():
            try:
                entries = iter(plan)        # _host_batches serves the plan in order: entry and batch go in step
                for size, ids, images, boxes, labels, counts, owner in self._host_batches(epoch, delivery, stop, plan):
                    entry = next(entries)
                    with torch.cuda.stream(copy_stream):
                        if on_device:
                            images = device_pixels.run(images, threads=min(self.num_threads, 8), cache=cache)
                        else:
                            images = images.to(dev, non_blocking=True)
                        bx = torch.from_numpy(boxes).pin_memory().to(dev, non_blocking=True)
                        lb = torch.from_numpy(labels.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
                        ct = torch.from_numpy(counts.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
                        if len(entry) > 3:      # mosaic: 4 * n samples -> n images, behind the pixels and the three uploads
                            images, bx, lb, ct = mosaic_batch(images, bx, lb, ct, entry[3], self.mosaic_min_side,
                                                              self.mosaic_min_visible)
                            ids = [ids[4 * j + own] for j, own in enumerate(entry[4])]
                        if affine is not None:  # every delivered image warped; the border is the letterbox padding's grey
                            images, bx, lb, ct = affine_batch(images, bx, lb, ct, self._affine_records(epoch, entry, affine),
                                                              pad_fill(), self.affine_min_side, self.affine_min_area,
                                                              self.affine_max_aspect)
                        ev = torch.cuda.Event()
                        ev.record(copy_stream)
                    if owner is not None:
                        owner[0].give(ev, owner[1])
                    put((ids, size, images, bx, lb, ct, ev))
                put(None)
            except BaseException as e:       # noqa: BLE001 - handed to the consumer
                put(e)

        th = threading.Thread(target=produce, name='y3-feeder', daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                ids, size, images, bx, lb, ct, ev = item
                torch.cuda.current_stream(dev).wait_event(ev)         # device-side ordering only
                for t in (images, bx, lb, ct):
                    t.record_stream(torch.cuda.current_stream(dev))
                out = Batch()
                out.image_ids, out.images, out.img_size = ids, images, size
                out.boxes, out.labels, out.counts = bx, lb, ct
                out.y_true = process_box_batch(bx, lb, ct, size, self.class_num, self.anchors, self.assign_iou_thresh)
                self.batches_served += 1
                yield out
        finally:
            stop.set()
            deadline = time.monotonic() + 30.0
            while th.is_alive() and time.monotonic() < deadline:      # drain what is queued so that nothing the producer
                try:                                                  # holds outlives the epoch (bounded: a worker that
                    q.get_nowait()                                    # never returns must not hang the caller's close())
                except queue.Empty:
                    th.join(timeout=0.05)
            while True:
                try:
                    q.get_nowait()
                except queue.Empty:
                    break
            copy_stream.synchronize()
            shared.close()

    def __iter__(self):
        return self.epoch(0)
