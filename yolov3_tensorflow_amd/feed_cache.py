# coding: utf-8
"""Decoded source images kept in HBM: what Feeder(cache_bytes=...) reads its sources from after their first use.

A training run reads the same files every epoch and a decoded image never changes, so each file is decoded once, its 8-bit
RGB pixels are copied into one device arena, and from then on the feed kernels read them where they lie
(y3f_plan_batch_src / y3_feed_run): for such an image the host decodes nothing, packs no source rectangle into the
batch's blob and uploads no pixels.  The arena is a torch tensor this object owns (the library allocates nothing), filled
front to back; nothing is ever evicted or moved, so an offset handed out stays valid for the life of the cache, and an
image that does not fit is left out for good and served packed, as without a cache.

Threads: `shape_of` may be called from any thread (the feeder's workers ask it before they open a file); everything else
belongs to the feeder's coordinator thread.  Ordering: an insert's copy goes onto torch's CURRENT stream - the feeder's
side stream, the one that later runs y3_feed_run - and stream order is all that is needed.
"""
import numpy as np

ALIGN = 16


class SourceCache(object):
    def __init__(self, device, capacity_bytes):
        import torch
        self.device = torch.device(device)
        self.capacity = int(capacity_bytes)
        if self.capacity <= 0:
            raise ValueError("SourceCache: capacity_bytes must be positive")
        self.arena = None           # uint8 [capacity], allocated on the first insert
        self.index = {}             # key -> (offset, h, w)
        self.refused = set()        # keys that did not fit
        self.used = 0
        self.hits = self.misses = self.bytes_refused = 0
        self._chunk, self._chunk_used, self._busy = None, 0, []       # pinned staging: the chunk being filled, retired ones

    def shape_of(self, key):
        """(h, w) of a cached image, or None."""
        entry = self.index.get(key)
        return None if entry is None else (entry[1], entry[2])

    def _stage(self, nbytes):
        """A pinned slice of nbytes that no earlier copy is still reading."""
        import torch
        if self._chunk is None or self._chunk_used + nbytes > self._chunk.numel():
            if self._chunk is not None:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))       # behind every copy out of that chunk
                self._busy.append((ev, self._chunk))
            free = [i for i, (ev, t) in enumerate(self._busy) if t.numel() >= nbytes and ev.query()]
            self._chunk = self._busy.pop(free[0])[1] if free else torch.empty(max(nbytes, 16 << 20), dtype=torch.uint8).pin_memory()
            self._chunk_used = 0
        view = self._chunk[self._chunk_used:self._chunk_used + nbytes]
        self._chunk_used += (nbytes + ALIGN - 1) // ALIGN * ALIGN
        return view

    def _insert(self, key, img):
        import torch
        h, w = img.shape[:2]
        nbytes = h * w * 3
        offset = (self.used + ALIGN - 1) // ALIGN * ALIGN
        if offset + nbytes > self.capacity:
            self.refused.add(key)
            self.bytes_refused += nbytes
            return None
        if self.arena is None:
            self.arena = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        pinned = self._stage(nbytes)
        pinned.numpy()[:] = np.ascontiguousarray(img, np.uint8).reshape(-1)
        self.arena[offset:offset + nbytes].copy_(pinned, non_blocking=True)
        self.used = offset + nbytes
        entry = self.index[key] = (offset, h, w)
        return entry

    def resolve(self, key, img):
        """The arena offset of one source of a job, or None (serve it packed).  img None: the job refers to the cache (a
        hit).  Otherwise the source was decoded (a miss) and is inserted here unless it already is in the index - a path
        decoded for two jobs before its first insert - or was refused before."""
        if key is None:
            return None
        entry = self.index.get(key)
        if img is None:
            if entry is None:
                raise KeyError("SourceCache: %r is referred to but not cached" % (key,))
            self.hits += 1
            return entry[0]
        self.misses += 1
        if entry is None and key not in self.refused:
            entry = self._insert(key, img)
        return None if entry is None else entry[0]

    def stats(self):
        return dict(hits=self.hits, misses=self.misses, images=len(self.index), bytes_used=self.used,
                    bytes_refused=self.bytes_refused)
