"""Host-only: the image-range planner of the fp32 conv launchers (y3_conv_image_ranges) and the scratch / block-count
queries that must agree with the launches it cuts.  One launch takes tensors below 2^29 elements; a larger call runs as
several launches over consecutive image ranges.  The test hook y3_debug_conv_range_limit lowers the limit so that small shapes
are cut; every test restores it."""
import contextlib
import ctypes

import pytest

LIMIT = 1 << 29
MAXR = 256


@pytest.fixture(scope='module')
def L():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def desc(n, h, w, cin, cout, k, stride, c_up=0):
    from yolov3_tensorflow_amd import _lib
    return _lib.ConvDesc(n, h, w, cin, c_up, cout, k, stride, 0)


def ranges(L, d, dz_stride=0, limit=LIMIT, max_ranges=MAXR):
    begin, count = (ctypes.c_int * max_ranges)(), (ctypes.c_int * max_ranges)()
    nr = L.y3_conv_image_ranges(ctypes.byref(d), dz_stride, limit, max_ranges, begin, count)
    return nr, list(begin[:max(nr, 0)]), list(count[:max(nr, 0)])


@contextlib.contextmanager
def lowered(L, elements):
    L.y3_debug_conv_range_limit(elements)
    try:
        yield
    finally:
        L.y3_debug_conv_range_limit(0)


def sizes(d, dz_stride, n):
    co = dz_stride if dz_stride > 0 else d.cout
    return n * d.h * d.w * d.cin, n * (d.h // d.stride) * (d.w // d.stride) * co


CASES = [
    # (desc, dz_stride, limit)
    (desc(64, 512, 512, 3, 32, 3, 1), 0, LIMIT),          # the stem at the first refused scale: the output is exactly 2^29
    (desc(64, 608, 608, 3, 32, 3, 1), 0, LIMIT),
    (desc(64, 608, 608, 32, 64, 3, 2), 0, LIMIT),         # layer 1: the input is over, the output is not
    (desc(64, 608, 608, 32, 64, 3, 2), 64, LIMIT),        # ... its gradients
    (desc(128, 416, 416, 32, 64, 3, 2), 64, LIMIT),
    (desc(5, 32, 32, 32, 64, 3, 1), 0, 100000),           # 5 images, two per range: 2 + 2 + 1
    (desc(5, 48, 32, 64, 32, 1, 1), 0, 200000),
    (desc(7, 26, 26, 256, 255, 1, 1), 256, 400000),       # a padded gradient row decides
    (desc(9, 16, 16, 32, 32, 3, 1), 0, 16 * 16 * 32 + 1), # one image per range
    (desc(200, 8, 8, 32, 32, 1, 1), 0, 8 * 8 * 32 + 1),   # 200 ranges
]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_ranges_are_disjoint_ordered_cover_the_batch_and_stay_under_the_limit(L, case):
    d, dzs, limit = CASES[case]
    nr, begin, count = ranges(L, d, dzs, limit)
    assert nr >= 1
    assert begin[0] == 0 and all(c > 0 for c in count)
    assert all(begin[i + 1] == begin[i] + count[i] for i in range(nr - 1))      # ordered, disjoint, no gap
    assert begin[-1] + count[-1] == d.n
    for c in count:
        a, b = sizes(d, dzs, c)
        assert a < limit and b < limit
    # as few as possible: one range fewer cannot hold the batch; near-equal: sizes differ by at most one, larger ones first
    per_image = max(sizes(d, dzs, 1))
    most = (limit - 1) // per_image
    assert nr == -(-d.n // most)
    assert max(count) - min(count) <= 1 and count == sorted(count, reverse=True)


def test_one_range_exactly_when_the_single_launch_check_passes(L):
    """The check the launchers made before they could cut: both tensors strictly below 2^29 elements."""
    for n, s, cin, cout, k, stride, dzs in [
            (64, 480, 3, 32, 3, 1, 0), (64, 512, 3, 32, 3, 1, 0), (64, 480, 32, 64, 3, 2, 0), (64, 512, 32, 64, 3, 2, 0),
            (64, 480, 32, 64, 3, 2, 64), (64, 512, 32, 64, 3, 2, 64), (64, 416, 32, 64, 3, 2, 0), (128, 416, 3, 32, 3, 1, 0),
            (32, 416, 3, 32, 3, 1, 0), (64, 208, 64, 32, 1, 1, 32), (8, 13, 1024, 255, 1, 1, 256)]:
        d = desc(n, s, s, cin, cout, k, stride)
        a, b = sizes(d, dzs, n)
        nr, _, count = ranges(L, d, dzs)
        assert (nr == 1) == (a < LIMIT and b < LIMIT), (n, s, cin, cout)
        if nr == 1:
            assert count == [n]
    # the two scales the issue names, at 32 channels
    assert ranges(L, desc(64, 480, 480, 32, 32, 1, 1))[0] == 1
    assert ranges(L, desc(64, 512, 512, 32, 32, 1, 1))[0] == 2          # 64 * 512^2 * 32 == 2^29: not below it
    assert ranges(L, desc(64, 512, 512, 32, 32, 1, 1))[2] == [32, 32]
    assert ranges(L, desc(64, 608, 608, 3, 32, 3, 1))[2] == [32, 32]
    assert ranges(L, desc(128, 416, 416, 3, 32, 3, 1))[2] == [64, 64]


def test_an_image_over_the_limit_and_bad_arguments_are_refused(L):
    from yolov3_tensorflow_amd import _lib
    d = desc(2, 64, 64, 32, 32, 1, 1)
    assert ranges(L, d, 0, 64 * 64 * 32)[0] == _lib.Y3_EINVAL            # one image == the limit: not below it
    assert b'one image' in L.y3_last_error()
    assert ranges(L, d, 0, 64 * 64 * 32 + 1)[0] == 2
    assert ranges(L, desc(1, 4096, 4096, 32, 32, 1, 1))[0] == _lib.Y3_EINVAL     # 2^29 elements in one image
    assert ranges(L, d, 64, 64 * 64 * 40)[0] == _lib.Y3_EINVAL           # the gradient's padded rows count
    for bad in (desc(0, 8, 8, 32, 32, 1, 1), desc(2, 8, 8, 32, 32, 1, 0), desc(2, 0, 8, 32, 32, 1, 1)):
        assert ranges(L, bad)[0] == _lib.Y3_EINVAL
    buf = (ctypes.c_int * 4)()
    assert L.y3_conv_image_ranges(None, 0, LIMIT, 4, buf, buf) == _lib.Y3_EINVAL
    assert L.y3_conv_image_ranges(ctypes.byref(d), 0, LIMIT, 4, None, buf) == _lib.Y3_EINVAL
    assert L.y3_conv_image_ranges(ctypes.byref(d), 0, 0, 4, buf, buf) == _lib.Y3_EINVAL


def test_max_ranges_is_honoured(L):
    from yolov3_tensorflow_amd import _lib
    d = desc(9, 16, 16, 32, 32, 3, 1)
    limit = 16 * 16 * 32 * 2 + 1                       # two images per range: 5 ranges
    guard = 12345
    for room in (5, 6):
        begin, count = (ctypes.c_int * 8)(*([guard] * 8)), (ctypes.c_int * 8)(*([guard] * 8))
        assert L.y3_conv_image_ranges(ctypes.byref(d), 0, limit, room, begin, count) == 5
        assert list(count[:5]) == [2, 2, 2, 2, 1] and list(begin[:5]) == [0, 2, 4, 6, 8]
        assert list(begin[5:]) == [guard] * 3 and list(count[5:]) == [guard] * 3        # nothing written past the ranges
    begin, count = (ctypes.c_int * 8)(*([guard] * 8)), (ctypes.c_int * 8)(*([guard] * 8))
    assert L.y3_conv_image_ranges(ctypes.byref(d), 0, limit, 4, begin, count) == _lib.Y3_EINVAL
    assert list(begin) == [guard] * 8 and list(count) == [guard] * 8                    # refused before anything is written
    assert L.y3_conv_image_ranges(ctypes.byref(d), 0, limit, 0, begin, count) == _lib.Y3_EINVAL


def test_the_hook_only_lowers_the_limit(L):
    d = desc(5, 32, 32, 32, 64, 3, 1)
    nb = lambda: L.y3_conv_stats_blocks(ctypes.byref(d), 0)
    whole = nb()
    assert whole == -(-5 * 32 * 32 // 128)
    with lowered(L, 150000):                           # two images per range (2 * 65536 elements of output)
        assert nb() == 2 * (2 * 32 * 32 // 128) + 32 * 32 // 128
        L.y3_debug_conv_range_limit((1 << 29) + 1)     # ignored: the lowered limit stays
        assert nb() == 2 * (2 * 32 * 32 // 128) + 32 * 32 // 128
        L.y3_debug_conv_range_limit(-5)                # ignored
        assert nb() == 2 * (2 * 32 * 32 // 128) + 32 * 32 // 128
    assert nb() == whole
    # the real limit cannot be raised: layer 1 at 64 x 512^2 stays two launches of 32 images whatever is asked for
    try:
        L.y3_debug_conv_range_limit(1 << 40)
        halves = L.y3_conv_stats_blocks(ctypes.byref(desc(32, 512, 512, 32, 64, 3, 2)), 0)
        assert L.y3_conv_stats_blocks(ctypes.byref(desc(64, 512, 512, 32, 64, 3, 2)), 0) == 2 * halves
        assert ranges(L, desc(64, 512, 512, 32, 64, 3, 2))[2] == [32, 32]
    finally:
        L.y3_debug_conv_range_limit(0)


def _split_count(L, d):
    return (L.y3_conv_wgrad_scratch_bytes(ctypes.byref(d)) - 256) // (d.k * d.k * d.cin * d.cout * 4)


def test_queries_under_a_lowered_limit_equal_what_the_ranges_need(L):
    """Statistics rows, fused BN-backward rows and the weight gradient's scratch of a cut launch: the SUM over the ranges of
    what each range's own launch needs (each range under the limit is an uncut launch, so the same query answers for it);
    the stream-K workspace: none, a cut launch never takes that schedule."""
    cases = [
        # (n, h, w, cin, cout, k, stride, limit)
        (5, 32, 32, 32, 64, 3, 1, 150000), (5, 48, 32, 32, 64, 3, 2, 150000), (5, 48, 32, 64, 32, 1, 1, 200000),
        (5, 32, 32, 256, 128, 1, 1, 600000), (7, 26, 26, 128, 256, 3, 1, 400000), (5, 20, 28, 32, 64, 3, 2, 40000),
        (5, 26, 26, 256, 255, 1, 1, 400000),
    ]
    for n, h, w, cin, cout, k, stride, limit in cases:
        d = desc(n, h, w, cin, cout, k, stride)
        dzs = -(-cout // 4) * 4
        _, _, counts_fwd = ranges(L, d, 0, limit)
        _, _, counts_wg = ranges(L, d, dzs, limit)
        _, _, counts_bn = ranges(L, d, -(-cout // 32) * 32, limit)
        assert len(counts_fwd) > 1 and len(counts_wg) > 1
        sub = lambda c: desc(c, h, w, cin, cout, k, stride)
        # per range, asked with the hook off: the launch of that range alone
        stats_parts = [L.y3_conv_stats_blocks(ctypes.byref(sub(c)), 0) for c in counts_fwd]
        bn_parts = [L.y3_conv_dgrad_bn_blocks(ctypes.byref(sub(c))) for c in counts_bn]
        wg_parts = [_split_count(L, sub(c)) for c in counts_wg]
        with lowered(L, limit):
            if cout % 4 == 0:
                assert L.y3_conv_stats_blocks(ctypes.byref(d), 0) == sum(stats_parts) > 0
            assert L.y3_conv_dgrad_bn_blocks(ctypes.byref(d)) == sum(bn_parts)
            assert (k == 1 and stride == 1) == (sum(bn_parts) > 0)
            assert _split_count(L, d) == sum(wg_parts)
            assert L.y3_conv_workspace_bytes(ctypes.byref(d)) == 0
            assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) != 1
    # the stem: one block of 27 x 32 partials per workgroup of every range (at most 1536 per range: one resident round), and
    # never less than the 4096 blocks the query has always reserved
    stem = desc(6, 96, 416, 3, 32, 3, 1)
    with lowered(L, 2 * 96 * 416 * 32 + 1):            # two images per range: 3 ranges of 768 pieces, one workgroup each
        assert L.y3_conv_wgrad_scratch_bytes(ctypes.byref(stem)) == 4096 * 27 * 32 * 4
    big = desc(64, 512, 512, 3, 32, 3, 1)              # 2 ranges of 32 images
    assert L.y3_conv_wgrad_scratch_bytes(ctypes.byref(big)) == 4096 * 27 * 32 * 4
    pieces = 8 * 512 * 4                               # a range of 8 images: 128-pixel pieces of its image rows
    groups = -(-pieces // -(-pieces // 1536))          # ... walked by at most 1536 workgroups, equal runs: 1490
    with lowered(L, 8 * 512 * 512 * 32 + 1):           # 8 such ranges
        assert L.y3_conv_wgrad_scratch_bytes(ctypes.byref(big)) == 8 * groups * 27 * 32 * 4 > 4096 * 27 * 32 * 4


def test_a_range_that_alone_would_take_stream_k_does_not(L):
    """y3_conv_schedule answers what runs: the whole launch (8 x 52 x 52, 128 -> 256) takes stream-K; cut in two, each range
    of four images alone would too (169 tiles), but a cut launch runs its ranges without a workspace."""
    d = desc(8, 52, 52, 128, 256, 3, 1)
    half = desc(4, 52, 52, 128, 256, 3, 1)
    assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) == 1
    assert L.y3_conv_schedule(ctypes.byref(half), 0, 1) == 1
    with lowered(L, 4 * 52 * 52 * 256 + 1):
        assert ranges(L, d, 0, 4 * 52 * 52 * 256 + 1)[2] == [4, 4]
        assert L.y3_conv_schedule(ctypes.byref(d), 0, 1) == 0
        assert L.y3_conv_workspace_bytes(ctypes.byref(d)) == 0
        assert L.y3_conv_schedule(ctypes.byref(half), 0, 1) == 1          # under the limit: an ordinary launch
    assert L.y3_conv_workspace_bytes(ctypes.byref(d)) > 0


@pytest.mark.parametrize('dtype', ['f32', 'f32_wino', 'f32_bf16x6', 'bf16'])
def test_the_train_workspace_query_follows_the_cut_layers(L, dtype):
    """y3_net_train_workspace_bytes (a dry run) goes through the same queries.  At 256 px, bs = 4 a limit of 3,000,000 elements
    cuts layers 0-3: their statistics and fused BN-backward rows round up per range and the weight gradients keep every range's
    splits, so the workspace can only grow (the peak may lie elsewhere and stay).  A batch-64 step at 512 and 608 px has a size."""
    from yolov3_tensorflow_amd import training, _lib
    from test_train_workspace_cpu import _Var
    from test_train_gpu import _conv_name
    topo = training._Topology(80)
    layer_vars = []
    for i, l in enumerate(topo.layers):
        base = _conv_name(i)
        w = _Var(base + '/weights', (l['k'], l['k'], l['cin'], l['cout']))
        if l['bn']:
            bn = tuple(_Var(base + '/BatchNorm/' + s, (l['cout'],), trainable=s in ('gamma', 'beta'))
                       for s in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
            layer_vars.append((w, bn, None))
        else:
            layer_vars.append((w, None, _Var(base + '/biases', (l['cout'],))))
    table, _ = training._var_table(layer_vars)
    net = ctypes.c_void_p()
    _lib.check(L.y3_net_create(None, 80, ctypes.byref(net)))
    try:
        _lib.check(L.y3_net_set_dtype(net, training._TRAIN_DTYPES[dtype]))
        whole = L.y3_net_train_workspace_bytes(net, table, 4, 256, 256)
        with lowered(L, 3000000):
            cut = L.y3_net_train_workspace_bytes(net, table, 4, 256, 256)
        assert 0 < whole <= cut < whole + (64 << 20)
        for size in (512, 608):
            assert L.y3_net_train_workspace_bytes(net, table, 64, size, size) > 64 * size * size * 32 * 4
    finally:
        L.y3_net_destroy(net)
