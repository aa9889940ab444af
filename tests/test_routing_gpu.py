"""The backward routing kernels of csrc/y3_train.hip, each on its own against an exact reference: y3_upsample2x_bwd,
y3_slice_accumulate, y3_pad_channels (numpy float32, bit for bit: y3_train.hip is built without FMA contraction or
fast-math) and y3_bias_grad (fp64 column sums, within the bound of its fp32 partial sums).  Outputs that are written, not
accumulated into, start as NaN: an element the kernel skips stays NaN and fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _env():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context(), fw.default_device()


def _at(t, elements):
    """device pointer `elements` floats into t"""
    return ctypes.c_void_p(t.data_ptr() + 4 * elements)


def _out(rng, shape, accumulate, dev):
    """(host copy of what the output holds before the call, device tensor): random when accumulating, NaN otherwise"""
    old = rng.standard_normal(shape).astype(np.float32) if accumulate else np.full(shape, np.nan, np.float32)
    return old, torch.from_numpy(old.copy()).to(dev)


# (n, h, w, c, g_channels, channel offset of the upsampled part inside g's rows)
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('n,h,w,c,gc,off', [
    (2, 3, 5, 8, 8, 0),
    (1, 13, 13, 128, 384, 128),        # g is a view into rows of 384 channels (the concat's gradient)
    (3, 4, 4, 4, 12, 4),               # one float4 per pixel, three images
    (2, 52, 52, 256, 256, 0),          # the route layer's shape at 416 x 416: 346,112 float4 outputs, 1352 full blocks
    # A work item is one float4 and the grid is capped at 4096 blocks of 256 threads: 1 x 105 x 105 x (384 / 4) = 1,058,400
    # float4 outputs > 1,048,576 threads, so the grid-stride loop turns, and it ends ragged: the second trip is 9824 items,
    # 38 blocks and 96 threads of the 39th.
    (1, 105, 105, 384, 384, 0),
])
def test_routing_upsample2x_bwd_is_the_2x2_sum(n, h, w, c, gc, off, accumulate):
    """dx[b,y,x,:] (+)= ((g00 + g01) + g10) + g11 over the 2x2 block (first index dy), in float32, bit for bit.
    Would catch: a wrong row stride (g_channels), a wrong pixel of the block, a dropped or forced `accumulate`, an element
    past the first grid pass left unwritten."""
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(n * 1000 + h * 10 + c + accumulate)
    g = rng.standard_normal((n, 2 * h, 2 * w, gc)).astype(np.float32)
    old, dx = _out(rng, (n, h, w, c), accumulate, dev)
    gd = torch.from_numpy(g).to(dev)
    _lib.check(L.y3_upsample2x_bwd(ctx, _at(gd, off), gc, n, h, w, c, accumulate, fw.ptr(dx)))
    gs = g[..., off:off + c]
    want = ((gs[:, 0::2, 0::2] + gs[:, 0::2, 1::2]) + gs[:, 1::2, 0::2]) + gs[:, 1::2, 1::2]
    if accumulate:
        want = old + want
    assert want.dtype == np.float32
    np.testing.assert_array_equal(dx.cpu().numpy(), want)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('rows,sc,off,c', [(7, 12, 4, 8), (338, 768, 256, 512), (5, 8, 0, 8), (1, 4, 0, 4), (3, 16, 12, 4)])
def test_routing_slice_accumulate_copies_or_adds_the_channel_slice(rows, sc, off, c, accumulate):
    """dst[r, 0:c] (+)= src[r, off:off+c], bit for bit.  Would catch: a wrong source row stride, a wrong channel offset, the
    last slice of a row (off + c == src_channels) read from the next row, a dropped or forced `accumulate`."""
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(rows + sc + off + c + accumulate)
    src = rng.standard_normal((rows, sc)).astype(np.float32)
    old, dst = _out(rng, (rows, c), accumulate, dev)
    srcd = torch.from_numpy(src).to(dev)
    _lib.check(L.y3_slice_accumulate(ctx, fw.ptr(srcd), sc, off, rows, c, accumulate, fw.ptr(dst)))
    want = src[:, off:off + c]
    np.testing.assert_array_equal(dst.cpu().numpy(), old + want if accumulate else want)


@pytest.mark.parametrize('rows,cs,cd', [(169, 255, 256), (10, 18, 32), (4, 75, 96), (3, 8, 8)])
def test_routing_pad_channels_zero_extends_every_row(rows, cs, cd):
    """dst[r, 0:c_src] = src[r, :], dst[r, c_src:] = 0 exactly (the output starts as NaN).  Would catch: rows read with the
    destination's stride, padding left unwritten or written with anything but zero."""
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(rows + cs + cd)
    src = rng.standard_normal((rows, cs)).astype(np.float32)
    _, dst = _out(rng, (rows, cd), 0, dev)
    srcd = torch.from_numpy(src).to(dev)
    _lib.check(L.y3_pad_channels(ctx, fw.ptr(srcd), cs, rows, cd, fw.ptr(dst)))
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:, :cs], src)
    assert got[:, cs:].size == rows * (cd - cs) and np.all(got[:, cs:] == 0.0)


@pytest.mark.parametrize('rows,c', [
    (338, 255), (1, 18),
    (600, 75),           # more rows than the 512 partial blocks: some blocks add two rows
    (5000, 300),         # c > 256: a thread owns two columns
])
def test_routing_bias_grad_is_the_column_sum(rows, c):
    """dbias[c] = sum over rows of dy[r, c] against the fp64 sum.  The bound is derived, not measured: with nb = min(rows, 512)
    partial blocks each partial is a sequential fp32 sum of at most ceil(rows / nb) terms, the partials are combined in fp64
    and the result is rounded once, so per column |err| <= (ceil(rows / nb) + 1) * 2^-24 * sum_r |dy[r, c]|.
    Run-to-run bit-exact.  Would catch: a column or a row left out or counted twice (an error of one term, ~1, against a
    bound of ~1e-4), a wrong row stride."""
    fw, _lib, L, ctx, dev = _env()
    rng = np.random.RandomState(rows + c)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    dyd = torch.from_numpy(dy).to(dev)
    scratch = torch.empty(1024 * c, device=dev)
    outs = []
    for _ in range(2):
        db = torch.full((c,), float('nan'), device=dev)
        _lib.check(L.y3_bias_grad(ctx, fw.ptr(dyd), rows, c, fw.ptr(db), fw.ptr(scratch)))
        outs.append(db.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    d64 = dy.astype(np.float64)
    nb = min(rows, 512)
    bound = (-(-rows // nb) + 1) * 2.0 ** -24 * np.abs(d64).sum(0)
    err = np.abs(outs[0].astype(np.float64) - d64.sum(0))
    assert np.all(err <= bound), 'column %d: %.3e > %.3e' % (int(np.argmax(err - bound)), err.max(), bound[np.argmax(err - bound)])


def test_routing_kernels_refuse_shapes_they_cannot_take():
    """c % 4 != 0, offset + c > src_channels, g_channels < c, c_dst < c_src, no rows: ValueError, nothing launched."""
    fw, _lib, L, ctx, dev = _env()
    a, b = torch.zeros(4096, device=dev), torch.zeros(4096, device=dev)
    with pytest.raises(ValueError):
        _lib.check(L.y3_upsample2x_bwd(ctx, fw.ptr(a), 8, 1, 2, 2, 6, 0, fw.ptr(b)))            # c % 4 != 0
    with pytest.raises(ValueError):
        _lib.check(L.y3_upsample2x_bwd(ctx, fw.ptr(a), 4, 1, 2, 2, 8, 0, fw.ptr(b)))            # g_channels < c
    with pytest.raises(ValueError):
        _lib.check(L.y3_slice_accumulate(ctx, fw.ptr(a), 12, 0, 4, 6, 0, fw.ptr(b)))            # c % 4 != 0
    with pytest.raises(ValueError):
        _lib.check(L.y3_slice_accumulate(ctx, fw.ptr(a), 12, 8, 4, 8, 0, fw.ptr(b)))            # offset + c > src_channels
    with pytest.raises(ValueError):
        _lib.check(L.y3_pad_channels(ctx, fw.ptr(a), 8, 4, 4, fw.ptr(b)))                       # c_dst < c_src
    with pytest.raises(ValueError):
        _lib.check(L.y3_bias_grad(ctx, fw.ptr(a), 0, 8, fw.ptr(b), fw.ptr(b)))                  # no rows
    torch.cuda.synchronize()
    assert float(b.abs().sum()) == 0.0
