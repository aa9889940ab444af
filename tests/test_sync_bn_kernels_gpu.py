"""The two halves of the batch-norm finalizes (y3_bn_sync_*: include/yolo355.h, synchronised batch norm), per op.

Two shards of rows stand for two ranks: the sums half runs per shard into a buffer of its own, the buffers are added on the
device (what the all-reduce does), the finish half runs per shard on the sum - and everything is compared with fp64
BN + LeakyReLU + residual over the CONCATENATED rows, with the tolerances of tests/test_train_gpu.py::
test_bn_train_forward_backward (mean 1e-5, y 2e-5, moving statistics rtol 1e-5 / atol 1e-6, gradients 2e-4 of the tensor's
max).  The moving variance must carry the unbiased factor of the GLOBAL count; d gamma / d beta are each shard's own share:
their SUM is the gradient of the sum-loss the fp64 side differentiates.

With one shard and the buffer left alone, sums-then-finish must write the bits of the one-call entries."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))


def _ctx():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context()


def _case(rows, c, bf16_z):
    """fp64 autograd over all rows; z is first rounded to what the device stores"""
    rng = np.random.RandomState(rows + c)
    z0 = rng.standard_normal((rows, c)) * 2 + rng.standard_normal(c)
    zt = torch.tensor(z0, dtype=torch.float32)
    if bf16_z:
        zt = zt.to(torch.bfloat16)
    z = zt.to(torch.float64).requires_grad_(True)
    gamma = torch.tensor(rng.uniform(0.5, 1.5, c), dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(rng.normal(0, 0.3, c), dtype=torch.float64, requires_grad=True)
    resid = rng.standard_normal((rows, c))
    mean, var = z.mean(0), z.var(0, unbiased=False)
    u = (z - mean) * gamma / torch.sqrt(var + 1e-5) + beta
    y = torch.where(u > 0, u, 0.1 * u) + torch.tensor(resid)
    dy = rng.standard_normal((rows, c))
    y.backward(torch.tensor(dy))
    return dict(zt=zt, z=z, gamma=gamma, beta=beta, resid=resid, mean=mean.detach().numpy(), var=var.detach().numpy(),
                y=y.detach().numpy(), dy=dy)


class _Shard(object):
    """one rank's tensors and the calls of the four halves"""

    def __init__(self, case, lo, hi, bf16_z):
        fw, _lib, L, ctx = _ctx()
        dev = fw.default_device()
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
        self.rows, self.c, self.b16 = hi - lo, case['zt'].shape[1], 1 if bf16_z else 0
        c = self.c
        self.z = case['zt'][lo:hi].contiguous().to(dev)
        self.gamma, self.beta = f32(case['gamma'].detach().numpy()), f32(case['beta'].detach().numpy())
        self.resid, self.dy = f32(case['resid'][lo:hi]), f32(case['dy'][lo:hi])
        self.stats = torch.empty((4, c), device=dev)
        self.mm, self.mv = f32(np.full(c, 0.25)), f32(np.full(c, 2.0))
        self.sc = torch.empty(L.y3_bn_bwd_scratch_bytes(c), dtype=torch.uint8, device=dev)
        self.buf = torch.full((2 * c + 1,), float('nan'), dtype=torch.float64, device=dev)
        self.dgam, self.dbet = torch.empty(c, device=dev), torch.empty(c, device=dev)
        self.dz = torch.empty((self.rows, c), dtype=self.z.dtype, device=dev)

    def stats_sums(self):
        fw, _lib, L, ctx = _ctx()
        _lib.check(L.y3_bn_sync_stats_sums(ctx, fw.ptr(self.z), self.b16, None, 0, self.rows, self.c, fw.ptr(self.buf),
                                           fw.ptr(self.sc)))

    def stats_finish(self, buf):
        fw, _lib, L, ctx = _ctx()
        s = self.stats
        _lib.check(L.y3_bn_sync_stats_finish(ctx, fw.ptr(buf), self.c, fw.ptr(self.gamma), fw.ptr(self.beta), ctypes.c_float(1e-5),
                                             ctypes.c_float(0.9), fw.ptr(s[0]), fw.ptr(s[1]), fw.ptr(s[2]), fw.ptr(s[3]),
                                             fw.ptr(self.mm), fw.ptr(self.mv)))

    def apply(self):
        """y through the fp32 apply pass (the bf16 case widens its z: the apply passes are not what is under test, and an fp32
        y keeps the tolerance of the fp32 cases)"""
        fw, _lib, L, ctx = _ctx()
        y = torch.empty((self.rows, self.c), device=self.z.device)
        s = self.stats
        _lib.check(L.y3_bn_apply_fwd(ctx, fw.ptr(self.z.float().contiguous()), fw.ptr(s[2]), fw.ptr(s[3]), fw.ptr(self.resid),
                                     self.rows, self.c, 1, fw.ptr(y)))
        return y

    def bwd_sums(self):
        fw, _lib, L, ctx = _ctx()
        s = self.stats
        _lib.check(L.y3_bn_sync_bwd_sums(ctx, fw.ptr(self.z), self.b16, fw.ptr(self.dy), fw.ptr(s[2]), fw.ptr(s[3]), fw.ptr(s[0]),
                                         fw.ptr(s[1]), self.rows, self.c, None, 0, fw.ptr(self.dgam), fw.ptr(self.dbet),
                                         fw.ptr(self.buf), fw.ptr(self.sc)))

    def bwd_finish(self, buf):
        fw, _lib, L, ctx = _ctx()
        s = self.stats
        _lib.check(L.y3_bn_sync_bwd_finish(ctx, fw.ptr(self.z), self.b16, fw.ptr(self.dy), fw.ptr(self.gamma), fw.ptr(s[2]),
                                           fw.ptr(s[3]), fw.ptr(s[0]), fw.ptr(s[1]), self.rows, self.c, fw.ptr(buf),
                                           fw.ptr(self.dz), fw.ptr(self.sc)))


@pytest.mark.parametrize('rows0,rows1,c,bf16_z', [
    (18, 54, 1024, False),
    (3, 1, 256, False),         # fewer rows than a pass of the column reduction (4)
    (700, 1300, 12, False),     # C/4 = 3: 85 rows per pass, a ragged last pass in both shards
    (300, 300, 1028, False),    # C/4 = 257: two columns per thread
    (150, 106, 64, True),       # z (and dz) stored in bf16
])
def test_two_shards_through_the_halves_equal_fp64_batch_norm_over_all_rows(rows0, rows1, c, bf16_z):
    rows = rows0 + rows1
    case = _case(rows, c, bf16_z)
    shards = [_Shard(case, 0, rows0, bf16_z), _Shard(case, rows0, rows, bf16_z)]
    for s in shards:
        s.stats_sums()
    total = shards[0].buf + shards[1].buf            # the all-reduce
    assert float(total[2 * c]) == rows
    for s in shards:
        s.stats_finish(total)
    y = torch.cat([s.apply() for s in shards]).float().cpu().numpy()
    unb = case['var'] * rows / (rows - 1.0)          # the GLOBAL unbiased factor
    for s in shards:
        assert rel_err(s.stats[0].cpu().numpy(), case['mean']) < 1e-5
        np.testing.assert_allclose(s.mm.cpu().numpy(), 0.25 * 0.9 + case['mean'] * 0.1, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(s.mv.cpu().numpy(), 2.0 * 0.9 + unb * 0.1, rtol=1e-5, atol=1e-6)
    assert torch.equal(shards[0].stats, shards[1].stats)
    assert rel_err(y, case['y']) < 2e-5
    for s in shards:
        s.bwd_sums()
    total = shards[0].buf + shards[1].buf
    assert float(total[2 * c]) == rows
    for s in shards:
        s.bwd_finish(total)
    dz = torch.cat([s.dz for s in shards]).float().cpu().numpy()
    want = case['z'].grad.numpy()
    if bf16_z:
        # dz is STORED in bf16: got = round(want + e) with |e| < 2e-4 max|want| as in the fp32 cases, and rounding to nearest
        # moves a value by at most half a unit in the last of bf16's 8 significant bits: 2^-8 of itself
        e = 2e-4 * np.abs(want).max()
        assert (np.abs(dz - want) <= e + 2.0 ** -8 * (np.abs(want) + e)).all()
    else:
        assert rel_err(dz, want) < 2e-4
    # the parameter gradients stay local: the two shards' shares ADD to the gradient over all rows
    assert rel_err((shards[0].dgam + shards[1].dgam).cpu().numpy(), case['gamma'].grad.numpy()) < 2e-4
    assert rel_err((shards[0].dbet + shards[1].dbet).cpu().numpy(), case['beta'].grad.numpy()) < 2e-4


@pytest.mark.parametrize('rows,c,bf16_z', [(72, 1024, False), (3, 256, False), (2000, 12, False), (600, 1028, False),
                                           (256, 64, True)])
def test_one_shard_with_the_buffer_untouched_is_the_one_call_entry_bit_for_bit(rows, c, bf16_z):
    fw, _lib, L, ctx = _ctx()
    case = _case(rows, c, bf16_z)
    a, b = _Shard(case, 0, rows, bf16_z), _Shard(case, 0, rows, bf16_z)
    # forward: the one-call entry reads fp32 z (the bf16 train step takes its sums from the conv epilogue): the bf16 case
    # gives it the same values widened
    z32 = a.z.float().contiguous()
    s = a.stats
    _lib.check(L.y3_bn_train_stats(ctx, fw.ptr(z32), rows, c, fw.ptr(a.gamma), fw.ptr(a.beta), ctypes.c_float(1e-5),
                                   ctypes.c_float(0.9), fw.ptr(s[0]), fw.ptr(s[1]), fw.ptr(s[2]), fw.ptr(s[3]), fw.ptr(a.mm),
                                   fw.ptr(a.mv), fw.ptr(a.sc)))
    b.stats_sums()
    b.stats_finish(b.buf)
    assert torch.equal(a.stats, b.stats) and torch.equal(a.mm, b.mm) and torch.equal(a.mv, b.mv)
    assert float(b.buf[2 * c]) == rows
    # ... and from the partial sums of a conv epilogue (here: rows of made-up partials)
    part = torch.tensor(np.random.RandomState(c).standard_normal((37, 2, c)) ** 2, dtype=torch.float32, device=a.z.device)
    pa, pb = _Shard(case, 0, rows, bf16_z), _Shard(case, 0, rows, bf16_z)
    s = pa.stats
    _lib.check(L.y3_bn_train_stats_partials(ctx, fw.ptr(part), 37, rows, c, fw.ptr(pa.gamma), fw.ptr(pa.beta), ctypes.c_float(1e-5),
                                            ctypes.c_float(0.9), fw.ptr(s[0]), fw.ptr(s[1]), fw.ptr(s[2]), fw.ptr(s[3]),
                                            fw.ptr(pa.mm), fw.ptr(pa.mv)))
    _lib.check(L.y3_bn_sync_stats_sums(ctx, None, 0, fw.ptr(part), 37, rows, c, fw.ptr(pb.buf), None))
    pb.stats_finish(pb.buf)
    assert torch.equal(pa.stats, pb.stats) and torch.equal(pa.mm, pb.mm) and torch.equal(pa.mv, pb.mv)
    # backward
    b.stats.copy_(a.stats)
    s = a.stats
    args = (fw.ptr(a.gamma), fw.ptr(s[2]), fw.ptr(s[3]), fw.ptr(s[0]), fw.ptr(s[1]), rows, c, fw.ptr(a.dgam), fw.ptr(a.dbet),
            fw.ptr(a.dz), fw.ptr(a.sc))
    if bf16_z:
        _lib.check(L.y3_bn_train_bwd_bf16(ctx, fw.ptr(a.z), fw.ptr(a.dy), *args))
    else:
        _lib.check(L.y3_bn_train_bwd(ctx, fw.ptr(a.z), fw.ptr(a.dy), *args))
    b.bwd_sums()
    b.bwd_finish(b.buf)
    assert torch.equal(a.dz, b.dz) and torch.equal(a.dgam, b.dgam) and torch.equal(a.dbet, b.dbet)
