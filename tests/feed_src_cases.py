"""By-reference forms of feed_cases.random_case jobs: shared by tests/test_feed_src_cpu.py (host run of the device
functions) and tests/test_feed_src_gpu.py (the kernels).  An arena is a uint8 buffer poisoned with 0xA5 in which whole
source images lie at shuffled, 16-aligned offsets with gaps between them.  Runner (GPU tests only) calls y3_feed_run on such a
plan, or on a packed one."""
import ctypes

import numpy as np

POISON = 0xA5


def place(rng, cases, cache_all=False):
    """cases -> (arena uint8 array, src1, src2): per case the arena offset of img1 / img2 or None (not in the arena).
    Unless cache_all, a third of the single sources is left out, and of every mix-up pair exactly one member (alternating)."""
    wanted = []                 # (case index, 1 or 2)
    pairs = 0
    for i, c in enumerate(cases):
        if c['img2'] is not None and not cache_all:
            wanted.append((i, 1 + pairs % 2))
            pairs += 1
        elif cache_all or i % 3 != 0:
            wanted += [(i, 1)] + ([(i, 2)] if c['img2'] is not None else [])
    order = [wanted[k] for k in rng.permutation(len(wanted))]
    src1, src2 = [None] * len(cases), [None] * len(cases)
    chunks, at = [], 16 * int(rng.randint(0, 4))
    for i, which in order:
        img = cases[i]['img%d' % which]
        (src1 if which == 1 else src2)[i] = at
        chunks.append((at, img))
        at += (img.size + 15) // 16 * 16 + 16 * int(rng.randint(0, 4))
    arena = np.full(max(at, 16), POISON, np.uint8)
    for off, img in chunks:
        arena[off:off + img.size] = img.reshape(-1)
    return arena, src1, src2


def ref_jobs(fn, cases, src1, src2):
    """The PixelJobs of `cases` with every source that has an arena offset replaced by a reference (NULL pointer)."""
    pjs = []
    for c, o1, o2 in zip(cases, src1, src2):
        kw = dict(c)
        if o1 is not None:
            kw['img1'] = fn.SourceRef('img1', *c['img1'].shape[:2])
        if o2 is not None:
            kw['img2'] = fn.SourceRef('img2', *c['img2'].shape[:2])
        pjs.append(fn.make_job(**kw))
    return pjs


class Runner(object):
    """y3_feed_run on a plan of feed_native.plan_batch(..., src1, src2) and a numpy arena."""

    def __init__(self):
        import torch
        from yolov3_tensorflow_amd import _lib, feed_native
        from yolov3_tensorflow_amd import framework as fw
        self.lib, self._lib, self.fn, self.ctx = _lib.lib(), _lib, feed_native, fw.context()
        self.tables = torch.from_numpy(feed_native.device_tables()).cuda()

    def plan(self, cases, arena, src1, src2):
        import torch
        blob, scratch_bytes, recs = self.fn.plan_batch(ref_jobs(self.fn, cases, src1, src2), src1=src1, src2=src2)
        n = len(cases)
        ow, oh = cases[0]['out_size']
        return dict(blob=blob, recs=recs, n=n, oh=oh, ow=ow, dev_blob=torch.from_numpy(blob).cuda(),
                    arena=torch.from_numpy(arena).cuda(),
                    scratch=torch.full((scratch_bytes + 16 + n * 208,), 0xA5, dtype=torch.uint8, device='cuda'),
                    out=torch.full((n, oh, ow, 3), float('nan'), device='cuda'))

    def call(self, p, recs=None, blob_bytes=None, arena=True, src_bytes=None, blob=True, scratch_bytes=None, out_hw=None):
        """The status of one call; recs: a host copy of the records to pass in place of the blob's; arena / blob False: NULL."""
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        oh, ow = (p['oh'], p['ow']) if out_hw is None else out_hw
        return self.lib.y3_feed_run(
            self.ctx, ptr(p['dev_blob']) if blob else None, p['blob'].size if blob_bytes is None else blob_bytes,
            ctypes.c_void_p(p['blob'].ctypes.data if recs is None else ctypes.addressof(recs)), p['n'], ptr(self.tables),
            ptr(p['scratch']), p['scratch'].numel() if scratch_bytes is None else scratch_bytes, ptr(p['arena']) if arena else None,
            p['arena'].numel() if src_bytes is None else src_bytes, ptr(p['out']), oh, ow)
