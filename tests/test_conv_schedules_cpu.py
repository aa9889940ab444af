"""Host-only: the schedule the fp32 conv launchers pick (y3_conv_schedule: use_streamk and the data-parallel launcher's own
grid choice, asked without launching) and the weight gradient's split count, pinned for the shapes of
tests/test_conv_schedules_gpu.py (tests/conv_schedule_cases.py).  A change to a schedule rule shows up here as a diff; the
GPU cases then have to move so that they still reach the path they are named for."""
import ctypes

import pytest

import conv_schedule_cases as C


@pytest.fixture(scope='module')
def L():
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_weight_gradient_splits_have_several_k_steps(L):
    got = []
    for (n, h, w, k, s, cin, cout, _, ragged), (ns_want, chunk_want) in zip(C.WGRAD, C.WGRAD_SPLITS):
        ns, chunk, last, _ = C.wgrad_split(L, n, h, w, k, s, cin, cout)
        got.append((ns, chunk))
        assert chunk > 1 and ns > 1
        if ragged is not None:
            assert last == ragged < chunk
    assert got == C.WGRAD_SPLITS
    # every case of test_train_gpu.test_conv_wgrad_and_dgrad_match_autograd gets ONE K-step per split (why these cases exist)
    for n, h, w, k, s, cin, cout in ((2, 20, 28, 3, 1, 64, 128), (2, 13, 13, 1, 1, 256, 255), (3, 16, 24, 3, 2, 32, 64)):
        assert C.wgrad_split(L, n, h, w, k, s, cin, cout)[1] == 1
    assert C.wgrad_split(L, 3, 150, 146, 1, 1, 64, 32)[3] == 4      # the ragged K-step: 4 of 32 pixels


def test_data_gradient_schedules(L):
    for n, h, w, cin, cout in C.DGRAD_S1:
        assert C.schedule(L, n, h, w, cout, 0, cin, 3, 1, 0, 1) == C.STREAMK
        assert C.schedule(L, n, h, w, cout, 0, cin, 3, 1, 0, 0) == C.ONE_PER_TILE
    for n, h, w, cin, cout, want in C.DGRAD_S2:
        got = tuple(C.schedule(L, n, h // 2, w // 2, cout, 0, cin, 3, 1, t, 1) for t in C.PARITY_TAPS)
        assert got == want
        assert all(C.schedule(L, n, h // 2, w // 2, cout, 0, cin, 3, 1, t, 0) == C.ONE_PER_TILE for t in C.PARITY_TAPS)
    # fwd Cin = 64 (Cout' < 128): no stream-K however many tiles; the shapes of the per-kernel test in test_train_gpu.py neither
    assert C.schedule(L, 3, 37, 37, 128, 0, 64, 3, 1, 0, 1) == C.ONE_PER_TILE
    assert C.schedule(L, 2, 20, 28, 128, 0, 64, 3, 1, 0, 1) == C.ONE_PER_TILE
    assert C.schedule(L, 2, 6, 6, 256, 0, 128, 3, 1, 4, 1) == C.ONE_PER_TILE


def test_resident_walk_thresholds(L):
    for name, n, h, w, cin, c_up, cout, _, want in C.FWD:
        assert C.schedule(L, n, h, w, cin, c_up, cout, 1, 1) == want, name
    n, h, w, cin, cout = C.FWD_STATS
    assert C.schedule(L, n, h, w, cin, 0, cout, 1, 1) == C.RESIDENT
    # the walk belongs to the 64x64 tiles: Cout <= 64 takes the 128-row tiles, a 3x3 conv the 128x128 tile
    assert C.schedule(L, 3, 150, 146, 32, 0, 64, 1, 1) == C.ONE_PER_TILE
    assert C.schedule(L, 8, 52, 52, 32, 0, 64, 3, 1, 0, 0) == C.ONE_PER_TILE
    # the largest 1x1 grid of test_conv_gpu.py (216 tiles) is far below it
    assert C.schedule(L, 3, 20, 28, 1024, 0, 512, 1, 1) == C.ONE_PER_TILE


def test_fused_bn_backward_cases(L):
    for n, h, w, cin, cout, dzs, bm, want in C.DGRAD_BN:
        assert C.schedule(L, n, h, w, dzs, 0, cin, 1, 1) == want
        blocks = L.y3_conv_dgrad_bn_blocks(ctypes.byref(C.desc(n, h, w, cin, 0, cout, 1, 1)))
        assert blocks == -(-(n * h * w) // bm)
    for bad in (C.desc(3, 20, 28, 64, 0, 128, 3, 1), C.desc(3, 20, 28, 64, 0, 128, 3, 2), C.desc(3, 20, 28, 64, 32, 128, 1, 1),
                C.desc(3, 20, 28, 66, 0, 128, 1, 1)):
        assert L.y3_conv_dgrad_bn_blocks(ctypes.byref(bad)) == 0
    assert L.y3_conv_dgrad_bn_blocks(None) == 0


def test_schedule_query_rejects_what_no_launcher_takes(L):
    assert L.y3_conv_schedule(None, 0, 1) == 0
    assert C.schedule(L, 2, 26, 26, 128, 0, 256, 5, 1) == 0           # kernel size
    assert C.schedule(L, 2, 26, 26, 128, 0, 256, 3, 1, 3, 1) == 0     # no parity class has three taps
    assert C.schedule(L, 32, 52, 52, 3, 0, 32, 3, 1) == 0             # the stem: one thread per pixel
    # the forward 3x3 convs of the 52 grid at batch 8 and 32 (what y3_net_layer_is_streamk reports per layer)
    assert C.schedule(L, 8, 52, 52, 128, 0, 256, 3, 1, 0, 1) == C.STREAMK
    assert C.schedule(L, 8, 52, 52, 128, 0, 256, 3, 1, 0, 0) == C.ONE_PER_TILE


def test_host_answers_are_the_recorded_ones(L):
    """The row-block counts, schedules and workspace sizes the net sizes its buffers by, against the table recorded ahead of
    the one-tile-table refactor (conv_schedule_cases.HOST_ANSWERS): a retile that changes a launcher and not the count that
    goes with it, or the other way round, shows up here at every branch of the ladders, without a device."""
    wrong = []
    for fn, shape, extra, limit, want in C.HOST_ANSWERS:
        if limit:
            L.y3_debug_conv_range_limit(limit)
        try:
            got = getattr(L, fn)(ctypes.byref(C.desc(*shape)), *extra)
        finally:
            if limit:
                L.y3_debug_conv_range_limit(0)
        if got != want:
            wrong.append((fn, shape, extra, limit, want, got))
    assert not wrong, wrong
    assert len(C.HOST_ANSWERS) == 134


def test_weight_gradient_host_answers_are_the_recorded_ones(L):
    """The scratch sizes of the three weight-gradient families and the Winograd eligibility, against the table recorded ahead
    of the one-plan refactor of the fp32 weight gradient (conv_schedule_cases.WGRAD_HOST_ANSWERS): the launcher walks the plan
    the size query reads, so a split rule, a range cut or the stem's floor that moved shows up here, without a device."""
    wrong = []
    for fn, shape, extra, limit, want in C.WGRAD_HOST_ANSWERS:
        if limit:
            L.y3_debug_conv_range_limit(limit)
        try:
            got = getattr(L, fn)(ctypes.byref(C.desc(*shape)), *extra)
        finally:
            if limit:
                L.y3_debug_conv_range_limit(0)
        if got != want:
            wrong.append((fn, shape, extra, limit, want, got))
    assert not wrong, wrong
    assert len(C.WGRAD_HOST_ANSWERS) == 100


def test_train_workspace_bytes_are_the_recorded_ones(L):
    """y3_net_train_workspace_bytes (a dry run through every route and scratch query) for the four train dtypes, with and
    without the second stream, against conv_schedule_cases.TRAIN_WORKSPACE_ANSWERS."""
    from yolov3_tensorflow_amd import training, _lib
    from test_train_workspace_cpu import _Var
    from test_train_gpu import _conv_name
    layer_vars = []
    for i, l in enumerate(training._Topology(80).layers):
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
    _lib.check(L.y3_net_create(None, 80, ctypes.byref(net)))      # no context: sizing only
    wrong = []
    try:
        for dtype, n, size, side, limit, want in C.TRAIN_WORKSPACE_ANSWERS:
            _lib.check(L.y3_net_set_dtype(net, training._TRAIN_DTYPES[dtype]))
            # any non-null stream handle: the dry run only asks whether there is one
            _lib.check(L.y3_net_train_set_wgrad_stream(net, ctypes.c_void_p(0x1000) if side else None))
            if limit:
                L.y3_debug_conv_range_limit(limit)
            try:
                got = L.y3_net_train_workspace_bytes(net, table, n, size, size)
            finally:
                if limit:
                    L.y3_debug_conv_range_limit(0)
            if got != want:
                wrong.append((dtype, n, size, side, limit, want, got))
    finally:
        _lib.check(L.y3_net_train_set_wgrad_stream(net, None))
        L.y3_net_destroy(net)
    assert not wrong, wrong
    assert len(C.TRAIN_WORKSPACE_ANSWERS) == 32
