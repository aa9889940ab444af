"""GPU tests of the YOLOv3-SPP feature: the two pooling kernels against torch and the ordered fp32 sum (bit for bit), between
guard bands; the 1x1 conv at Cin = 2048 on every route; the SPP net's inference forward against its op-by-op composition and
the oracle; the default architecture unchanged; one whole train step against the fp64 SPP oracle; the Trainer end to end.
Oracle pieces and cases: tests/spp_cases.py.  Every tolerance is the one the default architecture's own test uses, imported
or quoted with its source."""
import ctypes

import numpy as np
import pytest
import torch

import spp_cases as sc
from conftest import COCO_ANCHORS, blob_images

pytestmark = pytest.mark.gpu

POOL_LAYER = 55          # the 1x1 conv that reads spp(output of layer 54)


def _env():
    from yolov3_tensorflow_amd import framework as fw, _lib
    return fw, _lib, _lib.lib(), fw.context(), fw.default_device()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------
_REF = {}      # (what, shape, kind, ...) -> reference, computed once and left unchanged


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


@pytest.mark.parametrize('kind', ['continuous', 'ties'])
@pytest.mark.parametrize('shape', sc.GPU_SHAPES, ids=str)
def test_spp_fwd_equals_torch_bit_for_bit(shape, kind):
    from yolov3_tensorflow_amd import engine
    fw, _lib, L, ctx, dev = _env()
    x = torch.from_numpy(sc.inputs(kind, shape, seed=3))
    want = _ref(('fwd', shape, kind), lambda: sc.spp_ref(x))
    for dt in (torch.float32, torch.bfloat16):
        got = engine.spp_fwd(x.to(dt).to(dev)).cpu()
        assert got.dtype == dt and torch.equal(_bits(got), _bits(want.to(dt))), dt


@pytest.mark.parametrize('kind', ['continuous', 'ties'])
@pytest.mark.parametrize('shape', sc.GPU_SHAPES, ids=str)
def test_spp_bwd_equals_the_ordered_sum_bit_for_bit(shape, kind):
    """dense and strided x (the last slot of a materialised spp(x)), fp32 and bf16, accumulate 0 and 1, each run twice"""
    from yolov3_tensorflow_amd import engine
    fw, _lib, L, ctx, dev = _env()
    n, h, w, c = shape
    xn, g = sc.inputs(kind, shape, seed=11), sc.gradients(shape, seed=12)
    dx0 = np.random.RandomState(13).standard_normal(shape).astype(np.float32)
    want = _ref(('bwd', shape, kind), lambda: (sc.bwd_ordered(xn, g), sc.bwd_ordered(xn, g, dx0)))
    gd = torch.from_numpy(g).to(dev)
    for dt in (torch.float32, torch.bfloat16):
        dense = torch.from_numpy(xn).to(dt).to(dev)
        pooled = engine.spp_fwd(dense)
        for x, stride in ((dense, None), (pooled[..., 3 * c:], 4 * c)):
            for acc in (0, 1):
                runs = []
                for _ in range(2):
                    into = torch.from_numpy(dx0).to(dev) if acc else None
                    runs.append(engine.spp_bwd(x, gd, accumulate_into=into, x_stride=stride).cpu())
                assert torch.equal(_bits(runs[0]), _bits(runs[1])), 'two runs differ'
                assert torch.equal(_bits(runs[0]), _bits(torch.from_numpy(want[acc]))), (dt, stride, acc)


def test_spp_entry_points_refuse_bad_arguments():
    fw, _lib, L, ctx, dev = _env()
    x = torch.zeros((1, 3, 3, 16), device=dev)
    out = torch.zeros((1, 3, 3, 64), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    E = _lib.Y3_EINVAL
    assert L.y3_spp_fwd(ctx, p(x), 0, 1, 3, 3, 12, p(out)) == E            # c % 8
    assert L.y3_spp_fwd(ctx, p(x), 0, 0, 3, 3, 16, p(out)) == E
    assert L.y3_spp_fwd(ctx, None, 0, 1, 3, 3, 16, p(out)) == E
    assert L.y3_spp_fwd(ctx, ctypes.c_void_p(x.data_ptr() + 4), 0, 1, 3, 3, 8, p(out)) == E      # alignment
    assert L.y3_spp_bwd(ctx, p(x), 8, 0, p(out), 1, 3, 3, 16, 0, p(x)) == E        # x_stride < c
    assert L.y3_spp_bwd(ctx, p(x), 20, 0, p(out), 1, 3, 3, 16, 0, p(x)) == E       # x_stride % 8
    assert L.y3_spp_bwd(ctx, p(x), 16, 0, None, 1, 3, 3, 16, 0, p(x)) == E
    assert L.y3_spp_fwd(ctx, p(x), 0, 1, 3, 3, 16, p(out)) == 0
    fw.check_context()


def test_spp_entry_points_between_guard_bands():
    """both entry points through tests/guarded.py (exact-size buffers at 16-byte alignment, both poison passes) at
    (2,7,5,520) and (1,13,13,512): the entries tests/spp_cases.py adds to the guard-band table, run by that module's own test"""
    import test_guard_bands_gpu as TG
    mine = [e for e in TG.TABLE if set(e.covers) & {'y3_spp_fwd', 'y3_spp_bwd'}]
    assert len(mine) == 4 * len(sc.GUARD_SHAPES) and not {'y3_spp_fwd', 'y3_spp_bwd'} & set(TG.EXCLUDED)
    for e in mine:
        TG.test_guard_bands(e)


# ---- the 1x1 conv 2048 -> 512, its data gradient and its weight gradient, on every route a net dtype can pick for it ---------
CONV = (2, 7, 5, 1, 1, 2048, 512)       # n, h, w, k, stride, cin, cout


@pytest.mark.parametrize('planes', [0, 3, 2])
def test_conv_2048_to_512_forward_fp32_routes(planes):
    """direct kernel and the split-plane kernels (net dtypes 0 / 4, 2, 3), tests/test_conv_gpu.py's check and TOL"""
    import test_conv_gpu as TC
    n, h, w, k, stride, cin, cout = CONV
    rng = np.random.RandomState(2048)
    x, wt, scale, shift = TC.make_case(rng, n, h, w, k, cin, cout)
    got = TC.run_gpu(x, wt, scale, shift, k, stride, True, planes=planes)
    TC.check(got, TC.ref_conv(x, wt, scale, shift, k, stride, True), '1x1 2048->512', planes)


def test_conv_2048_to_512_gradients_fp32_routes():
    """y3_conv_wgrad, y3_conv2d_dgrad and y3_conv2d_dgrad_split (planes 3 and 2) with tests/test_train_gpu.py's own case body
    and tolerances (2e-4; planes = 2: 5e-3); the data gradient's mirrored shape is 512 -> 2048 output channels"""
    import test_train_gpu as TT
    TT.test_conv_wgrad_and_dgrad_match_autograd(*CONV)


def test_conv_2048_to_512_bf16_inference_route():
    import test_bf16_gpu as TB
    n, h, w, k, stride, cin, cout = CONV
    TB.test_bf16_conv_matches_fp64_on_rounded_operands(n, h, w, k, stride, cin, cout, False, 0, 0)


def test_conv_2048_to_512_bf16_train_routes():
    """net dtype 1: the training forward, the data gradient (overwrite and accumulate) and the weight gradient, with the case
    bodies and gates of tests/test_train_bf16_kernels_gpu.py"""
    import test_train_bf16_kernels_gpu as TK
    TK.test_train_forward_z_and_its_column_partials(*CONV)
    for acc in (0, 1):
        TK.test_dgrad_writes_and_accumulates(*CONV, acc=acc)
    TK.test_wgrad(*CONV)


# ---- inference forward ---------------------------------------------------------------------------------------------------
def _fresh_spp_model(params, class_num=80, spp=True, **kw):
    import yolov3_tensorflow_amd as y3
    y3.reset_default_graph()
    model = y3.yolov3(class_num, COCO_ANCHORS, **kw)
    model.spp = spp
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    variables = y3.global_variables(scope='yolov3')
    assert len(variables) == (371 if spp else 366)
    for v in variables:
        v.assign(params[v.op_name])
    return model


def _blob_images_hw(seed, n, h, w):
    from test_train_gpu import _blob_images_hw as f
    return f(seed, n, h, w)


def _compose_wino(model, x, net):
    """The f32_wino plan op by op through the C ABI's per-op entries: per layer of the net's own table the kernel its route
    names - the fused stem, F(4x4,3x3) where y3_conv_wino44_preferred, F(2x2,3x3) where y3_conv_wino_eligible, else direct -
    with y3_spp_fwd in front of the pool layer."""
    from yolov3_tensorflow_amd import engine, training
    import yolov3_tensorflow_amd as y3
    fw, _lib, L, ctx, dev = _env()
    topo = training._Topology(model.class_num, 1)
    n, h, w, _ = x.shape
    variables = {v.op_name: v for v in y3.global_variables(scope='yolov3')}
    from test_train_gpu import _conv_name
    tens = {0: x}
    outs = {}
    i = 0
    nl = len(topo.layers)
    while i < nl:
        l = topo.layers[i]
        base = _conv_name(i)
        bn = tuple(variables['%s/BatchNorm/%s' % (base, s)] for s in ('gamma', 'beta', 'moving_mean', 'moving_variance')) if l['bn'] else None
        wp, scale, shift = engine.prepare_conv_params(variables[base + '/weights'], bn_vars=bn,
                                                      bias_var=None if l['bn'] else variables[base + '/biases'])
        src = tens[l['src']]
        if i == 0:      # the stem runs inside layer 1's launch (y3_net_layer_fused: 1, then 2)
            l1 = topo.layers[1]
            base1 = _conv_name(1)
            bn1 = tuple(variables['%s/BatchNorm/%s' % (base1, s)] for s in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
            wp1, scale1, shift1 = engine.prepare_conv_params(variables[base1 + '/weights'], bn_vars=bn1)
            y = torch.empty((n, h // 2, w // 2, l1['cout']), device=dev)
            _lib.check(L.y3_conv2d_fwd_stem_s2(ctx, n, h, w, fw.ptr(src), fw.ptr(variables[base + '/weights'].tensor), fw.ptr(scale),
                                               fw.ptr(shift), fw.ptr(wp1), fw.ptr(scale1), fw.ptr(shift1), fw.ptr(y)))
            tens[l1['dst']] = y
            i = 2
            continue
        if L.y3_net_layer_pool(net, i):
            src = engine.spp_fwd(src)
        res = tens[l['resid']] if l['resid'] >= 0 else None
        up = tens[l['up']] if l['up'] >= 0 else None
        d = _lib.ConvDesc(n, src.shape[1], src.shape[2], l['cin'], up.shape[3] if up is not None else 0, l['cout'], l['k'], l['stride'],
                          l['act'])
        wt = variables[base + '/weights'].tensor
        if L.y3_conv_wino44_preferred(ctypes.byref(d)):
            y = engine.conv2d_fwd_wino44(src, engine.pack_wino44(wt), scale, shift, l['cout'], bool(l['act']), residual=res)
        elif L.y3_conv_wino_eligible(ctypes.byref(d)):
            y = engine.conv2d_fwd_wino(src, engine.pack_wino(wt), scale, shift, l['cout'], bool(l['act']), residual=res)
        else:
            y = engine.conv2d_fwd(src, wp, scale, shift, l['k'], l['stride'], l['cout'], bool(l['act']), residual=res, x_up=up)
        tens[l['dst']] = y
        ext = topo.tensors[l['dst']]['ext']
        if ext >= 0:
            outs[ext] = y
        i += 1
    return [outs[0], outs[1], outs[2]]


@pytest.fixture
def spp_model(isolated_graph):
    params = sc.spp_params(80, seed=1)
    return _fresh_spp_model(params), params


def test_spp_forward_equals_its_op_by_op_composition(spp_model):
    """n = 2 at 224 x 160 (grids 7x5, 14x10, 28x20): the fused plan against y3_conv2d_fwd* + y3_spp_fwd composed op by op, bit for
    bit, in net dtypes 0 (f32) and 4 (f32_wino); as tests/test_forward_gpu.py::test_fused_plan_equals_op_by_op_composition"""
    import yolov3_tensorflow_amd as y3
    model, _ = spp_model
    fw, _lib, L, ctx, dev = _env()
    x = torch.from_numpy(_blob_images_hw(3, 2, 224, 160)).to(dev)
    with y3.variable_scope('yolov3'):
        fused = model.forward(x, False)
        composed = model.forward_composed(x)
        assert len(y3.global_variables(scope='yolov3')) == 371      # (the composed path created nothing)
        for a, b in zip(fused, composed):
            assert torch.equal(a, b)
        model.compute_dtype = 'f32_wino'
        fused = model.forward(x, False)
        h = ctypes.c_void_p()
        _lib.check(L.y3_net_create_arch(None, 80, 1, ctypes.byref(h)))      # (a net without a context: the tables only)
        try:
            assert L.y3_net_set_dtype(h, 4) == 0
            fused_flags = [L.y3_net_layer_fused(h, i, 2, 224, 160) for i in range(L.y3_net_num_layers(h))]
            assert fused_flags[:2] == [1, 2] and not any(fused_flags[2:])
            composed = _compose_wino(model, x, h)
        finally:
            L.y3_net_destroy(h)
    for a, b in zip(fused, composed):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', ['f32', 'f32_bf16x6', 'f32_wino'])
def test_spp_forward_matches_the_oracle(spp_model, dtype):
    """tests/test_forward_gpu.py::_cmp with its atol = 2e-4, rtol = 1e-4 against the fp64 oracle forward of spp_cases"""
    import yolov3_tensorflow_amd as y3
    from test_forward_gpu import _cmp
    model, params = spp_model
    model.compute_dtype = dtype
    x = _blob_images_hw(3, 2, 224, 160)
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, False)
    ref = _ref(('fwd_oracle',), lambda: sc.forward_spp(params, x, dtype=torch.float64))
    for i, (g, r) in enumerate(zip(fms, ref)):
        e = _cmp(g.cpu().numpy(), r, 'SPP feature_map_%d vs fp64 oracle (%s)' % (i + 1, dtype))
        print('SPP %s feature_map_%d: max err %.3e' % (dtype, i + 1, e))


def test_spp_forward_bf16_stays_within_the_drift_bounds(spp_model):
    """the bounds of tests/test_bf16_gpu.py::test_bf16_forward_tracks_the_fp32_oracle: max |d| <= 3 % of the largest logit,
    rms <= 2 %, against the fp32 oracle; run-to-run bit-exact; fp32 feature maps"""
    import yolov3_tensorflow_amd as y3
    model, params = spp_model
    x = _blob_images_hw(3, 2, 224, 160)
    ref = sc.forward_spp(params, x)
    model.compute_dtype = 'bf16'
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, False)
        again = model.forward(x, False)
    for i, (g, g2, r) in enumerate(zip(fms, again, ref)):
        assert g.dtype == torch.float32 and torch.equal(g, g2)
        g = g.cpu().numpy()
        rel = float(np.abs(g - r).max() / np.abs(r).max())
        rms = float(np.sqrt(((g - r) ** 2).mean()) / np.sqrt((r ** 2).mean()))
        print('SPP bf16 feature_map_%d: max err / max|ref| = %.3e, rms rel = %.3e' % (i + 1, rel, rms))
        assert np.isfinite(g).all() and rel < 0.03 and rms < 0.02


# ---- the default architecture is what it was -----------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_architecture_0_gives_the_bits_of_y3_net_create(dtype):
    """a net from y3_net_create and one from y3_net_create_arch(0): one forward at 64 x 64 and one train step's gradients"""
    import test_guard_bands_gpu as TG
    from oracle import train_ref
    g = TG.G()
    L = g.L
    n, h, w = 2, 64, 64
    det = 3 * (5 + TG.CLASSES)
    x = torch.from_numpy(np.random.RandomState(0).rand(n, h, w, 3).astype(np.float32)).to(g.dev)
    yts = [torch.from_numpy(y).to(g.dev) for y in train_ref.synthetic_targets(9, n, [w, h], TG.CLASSES, COCO_ANCHORS, max_boxes=6)]
    ancp = TG.host_f32(COCO_ANCHORS)
    opts = g._lib.TrainOpts(0.9, 0, 0, ctypes.cast(ancp, ctypes.POINTER(ctypes.c_float)))
    results = []
    for arch in (None, 0):
        net = TG._Net(g, dtype, trainable=True)
        if arch is not None:
            L.y3_net_destroy(net.h)
            net.h = ctypes.c_void_p()
            g._lib.check(L.y3_net_create_arch(g.ctx, TG.CLASSES, arch, ctypes.byref(net.h)))
            g._lib.check(L.y3_net_set_dtype(net.h, TG.NET_DTYPES[dtype]))
        assert L.y3_net_num_layers(net.h) == 75
        pb, wb = L.y3_net_params_bytes(net.h), L.y3_net_workspace_bytes(net.h, n, h, w)
        params, ws = torch.empty(pb, dtype=torch.uint8, device=g.dev), torch.empty(wb, dtype=torch.uint8, device=g.dev)
        fms = [torch.empty((n, h // s, w // s, det), device=g.dev) for s in (32, 16, 8)]
        g('y3_net_set_params', net.h, net.table, TG.P(params), ctypes.c_size_t(pb))
        g('y3_net_forward', net.h, TG.P(x), n, h, w, TG.P(ws), ctypes.c_size_t(wb), *[TG.P(f) for f in fms])
        tb = L.y3_net_train_workspace_bytes(net.h, net.table, n, h, w)
        tws = torch.empty(tb, dtype=torch.uint8, device=g.dev)
        flat, loss5 = torch.full((net.grad_elements,), float('nan'), device=g.dev), torch.empty(5, device=g.dev)
        g('y3_net_train_step', net.h, net.table, TG.P(x), n, h, w, TG.P(yts[0]), TG.P(yts[1]), TG.P(yts[2]), ctypes.byref(opts),
          TG.P(flat), TG.P(tws), ctypes.c_size_t(tb), TG.P(loss5), g._lib.GradReadyFn(), None)
        torch.cuda.synchronize()
        results.append((pb, wb, tb, [f.cpu() for f in fms], flat.cpu(), loss5.cpu()))
        net.destroy()
    a, b = results
    assert a[:3] == b[:3]
    for p, q in zip(a[3], b[3]):
        assert torch.equal(_bits(p), _bits(q))
    assert torch.isfinite(a[4]).all() and torch.equal(_bits(a[4]), _bits(b[4])) and torch.equal(_bits(a[5]), _bits(b[5]))


# ---- one whole train step against the fp64 SPP oracle ------------------------------------------------------------------------
def _head(j):
    from test_train_gpu import _conv_name
    return _conv_name(52 + j) + '/'


# what is updated: everything; the head; from the SPP conv up (head conv 3 = layer 55: no pool backward is launched); from the
# conv below it up (head conv 2 = layer 54: the pool backward writes the dy of a layer whose BN backward is then unfused)
UPDATE_SETS = {
    'all': None,
    'head': ['yolov3/yolov3_head/'],
    'from_spp_conv': [_head(j) for j in range(3, 24)],
    'from_conv_below': [_head(j) for j in range(2, 24)],
}


def _pool_argmax(model, n, gh, gw):
    """The first-max rule on the device's own x: the last slot of the spp(x) the forward kept (y3_net_train_saved_pool)"""
    fw, _lib, L, ctx, dev = _env()
    st = model._train
    off = ctypes.c_size_t()
    _lib.check(L.y3_net_train_saved_pool(st['net'], POOL_LAYER, ctypes.byref(off)))
    assert off.value != ctypes.c_size_t(-1).value
    for other in (0, 54, 56, 75):
        o2 = ctypes.c_size_t()
        _lib.check(L.y3_net_train_saved_pool(st['net'], other, ctypes.byref(o2)))
        assert o2.value == ctypes.c_size_t(-1).value
    half = model.compute_dtype == 'bf16'
    dt, es = (torch.bfloat16, 2) if half else (torch.float32, 4)
    pooled = st['ws'][off.value:off.value + n * gh * gw * 2048 * es].view(dt).view(n, gh, gw, 2048)
    x = pooled[..., 1536:].float().cpu()
    # the kept tensor is spp of its own last slot, bit for bit
    assert torch.equal(_bits(pooled.cpu()), _bits(sc.spp_ref(x.to(dt))))
    return {k: sc.first_argmax(x.numpy(), k) for k in sc.WINDOWS}


def _spp_step(optimizer, update, dtype, wgrad_stream, class_num=80, hw=(256, 256), bs=4, data_seeds=(21, 5), mix_up=None,
              box_loss='mse', ema_decay=None):
    """tests/test_train_gpu.py::_step_matches_oracle for the SPP architecture: the fp64 oracle takes the device's LeakyReLU
    branches and the device's pool argmax.  Returns what the caller gates: (trainer, loss, oracle step, params).
    run['raw_grads']: every gradient view as backward left it, before apply_gradients (lamb overwrites the views with its
    direction, every rule clips in place)."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    from oracle import train_ref
    from test_train_gpu import _conv_name
    params = sc.spp_params(class_num, seed=1)
    n, (h, w) = bs, hw
    x = blob_images(data_seeds[0], n, h) if h == w else _blob_images_hw(data_seeds[0], n, h, w)
    yts = train_ref.synthetic_targets(data_seeds[1], n, [w, h], class_num, COCO_ANCHORS, max_boxes=4, mix_up=mix_up)
    lr = 1e-3
    model = _fresh_spp_model(params, class_num, batch_norm_decay=0.99, weight_decay=5e-4)
    model.compute_dtype = dtype
    model.box_loss = box_loss
    prefixes = UPDATE_SETS[update]
    upd = None if prefixes is None else [v for v in y3.global_variables(scope='yolov3')
                                         if any(v.op_name.startswith(p) for p in prefixes)]
    trainer = training.Trainer(model, config_optimizer(optimizer, lr), update_vars=upd, wgrad_stream=wgrad_stream,
                               ema_decay=ema_decay)
    trainer.capture = []
    raw_grads = {}
    apply_gradients = trainer.apply_gradients

    def keep_then_apply():
        raw_grads.update({k: v.clone() for k, v in trainer.views.items()})
        apply_gradients()
    trainer.apply_gradients = keep_then_apply
    with y3.variable_scope('yolov3'):
        loss = trainer.step(x, yts)
    del trainer.apply_gradients
    masks = {}
    for rec in trainer.capture:
        if rec['z'] is not None:
            pos = (rec['z'].float() * rec['stats'][2] + rec['stats'][3]) > 0
            masks[_conv_name(rec['layer'])] = pos.permute(0, 3, 1, 2).cpu()
    trainer.capture = None
    argmax = _pool_argmax(model, n, h // 32, w // 32)
    return dict(trainer=trainer, model=model, loss=loss, params=params, x=x, yts=yts, masks=masks, argmax=argmax, lr=lr,
                raw_grads=raw_grads, names=None if upd is None else set(v.op_name for v in upd if v.trainable), class_num=class_num)


GRAD_TOL = 2e-4                      # tests/test_train_gpu.py::_step_matches_oracle
LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-6    # the same


def _gate_against_fp64(run, optimizer, what, min_iou_margin=None):
    """the gates of _step_matches_oracle: loss 1e-4, every gradient tensor GRAD_TOL = 2e-4, the updated variables and the
    moving statistics as there (sgd / momentum: 1e-4 of the tensor's scale plus the gradient tolerance times the step).
    min_iou_margin: as there, no record's ignore mask may hang on the precision of its IoU - asserted on this oracle run."""
    import yolov3_tensorflow_amd as y3
    from oracle import train_ref
    from test_train_gpu import rel_err
    trainer, params, lr = run['trainer'], run['params'], run['lr']
    ref = sc.train_step(params, run['x'], run['yts'], COCO_ANCHORS, class_num=run['class_num'], optimizer='sgd', lr=lr,
                        weight_decay=5e-4, bn_decay=0.99, update_names=run['names'], dtype=torch.float64, step=1,
                        masks=run['masks'], pool_argmax=run['argmax'])
    new_params = train_ref.reapply(params, ref, optimizer, lr, step=1)
    if min_iou_margin is not None:
        print('smallest |best IoU - 0.5| per scale: %s' % ref['iou_margins'])
        assert min(ref['iou_margins']) >= min_iou_margin, ref['iou_margins']
    for a, b in zip(run['loss'], ref['loss']):
        assert abs(float(a) - b) <= LOSS_RTOL * abs(b) + LOSS_ATOL, ([float(v) for v in run['loss']], ref['loss'])
    assert set(trainer.views) == set(ref['grads'])
    errs = {name: rel_err(trainer.views[name].cpu().numpy(), g) for name, g in ref['grads'].items()}
    worst = max(errs, key=errs.get)
    print('%s: gradient rel err vs the fp64 SPP oracle on the GPU\'s branches and argmax: worst %.2e (%s), median %.2e over %d tensors'
          % (what, errs[worst], worst, float(np.median(list(errs.values()))), len(errs)))
    for name, e in errs.items():
        assert e < GRAD_TOL, '%s: grad rel err %.3e' % (name, e)
    for v in y3.global_variables(scope='yolov3'):
        want, got = new_params[v.op_name], v.numpy()
        scale = max(np.abs(want).max(), 1e-6)
        slack = GRAD_TOL * lr * float(np.abs(ref['grads'][v.op_name]).max()) if v.op_name in ref['grads'] else 0.0
        assert np.abs(got - want).max() <= 1e-4 * scale + slack, v.op_name
        if v.op_name not in trainer.views and '/moving_' not in v.op_name:
            np.testing.assert_array_equal(got, params[v.op_name], err_msg=v.op_name)
    return errs


@pytest.mark.parametrize('optimizer,update,dtype', [
    ('sgd', 'all', 'f32'), ('momentum', 'all', 'f32_wino'), ('sgd', 'all', 'f32_bf16x6'),
    ('momentum', 'head', 'f32'), ('sgd', 'from_spp_conv', 'f32'), ('sgd', 'from_conv_below', 'f32')])
def test_spp_train_step_matches_the_fp64_oracle(optimizer, update, dtype, isolated_graph):
    """256 x 256 with bs = 4: an 8 x 8 grid, on which the three windows all differ, and 256 samples per BN channel"""
    run = _spp_step(optimizer, update, dtype, 'auto')
    n_vars = len(run['trainer'].views)
    assert n_vars == {'all': 225, 'head': 225 - 156, 'from_spp_conv': 225 - 156 - 9, 'from_conv_below': 225 - 156 - 6}[update]
    _gate_against_fp64(run, optimizer, '%s/%s/%s' % (optimizer, update, dtype))


def test_spp_train_step_off_the_square_matches_the_fp64_oracle(isolated_graph):
    """tests/test_train_gpu.py's OFF_SQUARE: 160 x 224 (grids 5x7, 10x14, 20x28), bs = 8, 20 classes, mix-up weights"""
    from test_train_gpu import OFF_SQUARE
    kw = {k: v for k, v in OFF_SQUARE.items() if k != 'min_iou_margin'}
    run = _spp_step('sgd', 'all', 'f32', 'auto', **kw)
    # OFF_SQUARE's precondition, on this network's feature maps: with these data seeds the fp64 SPP oracle on its own branches
    # keeps every record 1.1e-3, 4.7e-3 and 8.6e-3 from IoU 0.5 on the three scales (target seeds 1 and 4-7 on the same images:
    # 1.9e-4 to 5.0e-4 at the closest); asserted below on the run that takes the GPU's branches
    _gate_against_fp64(run, 'sgd', 'sgd/all/f32 off the square', min_iou_margin=OFF_SQUARE['min_iou_margin'])


def test_spp_train_step_bf16_stays_within_the_contract_tolerances(isolated_graph):
    """net dtype 1 against the bf16 contract oracle of tests/test_train_bf16_gpu.py with the SPP block mixed in (max is exact in
    bf16: the block adds no rounding of its own), at that test's CONTRACT_TOLS: feature maps, the loss at the GPU's feature
    maps, worst and median gradient tensor"""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training, framework as fw
    from oracle import train_ref
    from test_train_bf16_gpu import CONTRACT_TOLS, _contract_graph, l2_err
    from test_train_gpu import rel_err
    run = _spp_step('sgd', 'all', 'bf16', 'auto')
    model, trainer, params, x, yts = run['model'], run['trainer'], run['params'], run['x'], run['yts']

    class SppContract(sc.SppMixin, _contract_graph()):
        pass

    # the feature maps of the step's forward: a training forward with the variables as they were (bit-identical)
    probe = _fresh_spp_model(params, batch_norm_decay=0.99, weight_decay=5e-4)
    probe.compute_dtype = 'bf16'
    with y3.variable_scope('yolov3'):
        fm_gpu = [f.double().cpu() for f in training.forward_train(probe, fw.as_device_f32(x))]
    names = sorted(trainer.views)
    g = SppContract(params, 80, torch.float64, masks=run['masks'])
    g.pool_argmax = run['argmax']
    fms_o = g.forward(x)
    fl = [f.clone().requires_grad_(True) for f in fm_gpu]
    lo = g.compute_loss(fl, yts, COCO_ANCHORS)
    dfm = torch.autograd.grad(lo[0], fl)
    total = sum((fo * d).sum() for fo, d in zip(fms_o, dfm)) + g.l2_loss(5e-4)
    grads = torch.autograd.grad(total, [g.p[k] for k in names])
    ref = {k: train_ref.clip_by_norm(gr.double(), 100.0).numpy() for k, gr in zip(names, grads)}
    e_loss = max(abs(float(a) - float(b)) / max(abs(float(b)), 1e-6) for a, b in zip(run['loss'], lo))
    e_fm = max(l2_err(a.numpy(), b.detach().numpy()) for a, b in zip(fm_gpu, fms_o))
    errs = {k: rel_err(trainer.views[k].cpu().numpy(), ref[k]) for k in names}
    worst = max(errs, key=errs.get)
    med = float(np.median(list(errs.values())))
    print('SPP bf16: feature maps l2-relative %.2e from the contract oracle; loss at the GPU\'s feature maps %.2e; gradients worst '
          '%.2e (%s), median %.2e over %d tensors' % (e_fm, e_loss, errs[worst], worst, med, len(errs)))
    FM_TOL, LOSS_TOL, GRAD_TOL, GRAD_MED_TOL = CONTRACT_TOLS
    assert e_loss < LOSS_TOL and e_fm < FM_TOL
    assert errs[worst] < GRAD_TOL, '%s: grad rel err %.3e' % (worst, errs[worst])
    assert med < GRAD_MED_TOL


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_spp_weight_gradients_on_the_second_stream_change_no_bit(dtype, isolated_graph):
    from oracle import train_ref
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    params = sc.spp_params(80, seed=4)
    x = blob_images(7, 3, 128)
    yts = train_ref.synthetic_targets(8, 3, [128, 128], 80, COCO_ANCHORS, max_boxes=4)
    runs = []
    for side in (False, True):
        model = _fresh_spp_model(params, batch_norm_decay=0.99)
        model.compute_dtype = dtype
        trainer = training.Trainer(model, config_optimizer('momentum', 1e-3), wgrad_stream=side)
        with y3.variable_scope('yolov3'):
            losses = [float(trainer.step(x, yts)[0]) for _ in range(2)]
        torch.cuda.synchronize()
        runs.append((losses, trainer.flat.clone()))
    assert np.isfinite(runs[0][0]).all() and runs[0][0] == runs[1][0]
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize('dtype', ['f32_wino', 'bf16'])
def test_spp_backward_run_twice_from_one_forward_writes_the_same_bits(dtype, isolated_graph):
    """tests/test_train_gpu.py::test_backward_run_twice_from_one_forward_writes_the_same_bits on the SPP net: the materialised
    spp(x) stays with the forward, the pool backward has one fixed order"""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    from oracle import train_ref
    model = _fresh_spp_model(sc.spp_params(80, seed=4), batch_norm_decay=0.99)
    model.compute_dtype = dtype
    model.wgrad_stream = False
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), wgrad_stream=False)
    x = _blob_images_hw(21, 2, 96, 64)
    yts = train_ref.synthetic_targets(22, 2, [64, 96], 80, COCO_ANCHORS, max_boxes=3)
    flats = []
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, is_training=True)
        training.compute_loss(model, fms, yts)
        trainer._alloc_grads(model._train['layer_vars'], fms[0].device)
        for _ in range(2):
            trainer.flat.fill_(float('nan'))
            trainer.backward()
            torch.cuda.synchronize()
            for name, view in trainer.views.items():
                assert bool(torch.isfinite(view).all()), '%s: gradient not written' % name
            flats.append(trainer.flat.clone())
    assert torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32))


# ---- the scripts ---------------------------------------------------------------------------------------------------------
def test_scripts_take_the_spp_architecture(tmp_path, capsys, isolated_graph):
    """convert_weight.py --spp true on a darknet file in graph order (80 classes), train.py --spp true from the converted
    checkpoint on a 3-class set (the default --restore_exclude leaves out the detection convs under their SPP names), and
    eval.py --spp true on what train.py saved"""
    import os
    import sys
    import yolov3_tensorflow_amd as y3
    from oracle import yolo_ref
    from conftest import ROOT
    from test_train_script_gpu import make_dataset
    sys.path.insert(0, ROOT)
    import convert_weight
    import train as train_script
    import eval as eval_script
    params = sc.spp_params(80, seed=2)
    weights = str(tmp_path / 'yolov3-spp.weights')
    yolo_ref.write_darknet(params, weights)
    anchors = os.path.join(ROOT, 'data', 'yolo_anchors.txt')
    y3.reset_default_graph()
    ckpt = convert_weight.main(['--weight_path', weights, '--save_path', str(tmp_path / 'yolov3-spp.ckpt'), '--anchor_path', anchors,
                                '--spp', 'true'])
    stored = np.load(ckpt)
    assert len(stored.files) == 371
    for k, v in params.items():
        np.testing.assert_array_equal(stored[k], v, err_msg=k)
    ann, names = make_dataset(tmp_path)
    y3.reset_default_graph()
    hist = train_script.main([
        '--train_file', ann, '--val_file', ann, '--restore_path', ckpt, '--save_dir', str(tmp_path / 'ckpt'), '--progress_log_path', '',
        '--anchor_path', anchors, '--class_name_path', names, '--batch_size', '4', '--img_size', '64', '64', '--letterbox_resize',
        'false', '--total_epoches', '2', '--train_evaluation_step', '1000', '--val_evaluation_epoch', '1', '--batch_norm_decay', '0.9',
        '--save_epoch', '1000', '--optimizer_name', 'momentum', '--learning_rate_init', '1e-3', '--lr_type', 'fixed',
        '--multi_scale_train', 'false', '--use_warm_up', 'false', '--warm_up_epoch', '0', '--use_label_smooth', 'false',
        '--use_focal_loss', 'false', '--weight_decay', '0', '--augment', 'false', '--num_threads', '2', '--spp', 'true'])
    assert np.isfinite(hist['loss']).all() and len(hist['loss']) == 4
    names_now = [v.op_name for v in y3.global_variables(scope='yolov3')]
    assert len(names_now) == 371
    # restored by name: the body and the head but its detection convs (3 classes: another shape than the file's)
    body = y3.global_variables(scope='yolov3/darknet53_body')
    np.testing.assert_array_equal(body[0].numpy(), params[body[0].op_name])
    files = sorted(os.listdir(str(tmp_path / 'ckpt')))
    npz = [f for f in files if f.startswith('best_model_') and f.endswith('.npz')]
    assert npz
    capsys.readouterr()
    y3.reset_default_graph()
    out = eval_script.main(['--eval_file', ann, '--restore_path', str(tmp_path / 'ckpt' / npz[-1]), '--anchor_path', anchors,
                            '--class_name_path', names, '--img_size', '64', '64', '--batch_size', '8', '--num_threads', '2',
                            '--compute_dtype', 'f32', '--spp', 'true'])
    assert 'final mAP' in capsys.readouterr().out and np.isfinite(out['loss']).all()
    # the same file without --spp does not fit: the error names the first variable whose shape differs
    y3.reset_default_graph()
    with pytest.raises(ValueError) as err:
        eval_script.main(['--eval_file', ann, '--restore_path', str(tmp_path / 'ckpt' / npz[-1]), '--anchor_path', anchors,
                          '--class_name_path', names, '--img_size', '64', '64', '--batch_size', '8', '--num_threads', '2',
                          '--compute_dtype', 'f32'])
    assert 'yolov3/yolov3_head/Conv_3/weights' in str(err.value)
    # test_single_image.py has no --spp option: tools/run_spp.py runs it on the SPP architecture, with its own arguments; run
    # directly, it builds the default architecture and refuses the file at the same variable
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_spp
    import test_single_image
    single = [str(tmp_path / 't0.png'), '--anchor_path', anchors, '--class_name_path', names, '--new_size', '64', '64',
              '--restore_path', str(tmp_path / 'ckpt' / npz[-1]), '--compute_dtype', 'f32']
    y3.reset_default_graph()
    boxes, scores, labels = run_spp.main(['test_single_image.py'] + single)
    assert len(y3.global_variables(scope='yolov3')) == 371 and boxes.shape[1:] == (4,) and len(scores) == len(labels) == len(boxes)
    assert y3.yolov3.default_spp is False
    y3.reset_default_graph()
    with pytest.raises(ValueError) as err:
        test_single_image.main(single)
    assert 'yolov3/yolov3_head/Conv_3/weights' in str(err.value)
    with pytest.raises(SystemExit):
        run_spp.main(['train.py'])


# ---- the Trainer end to end --------------------------------------------------------------------------------------------------
def test_spp_trainer_three_lamb_steps_with_averaging_then_checkpoint_and_restore(isolated_graph, tmp_path):
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer, Saver, EMA_SUFFIX
    from oracle import train_ref
    params = sc.spp_params(80, seed=2)
    x = blob_images(4, 2, 96)
    yts = train_ref.synthetic_targets(6, 2, [96, 96], 80, COCO_ANCHORS, max_boxes=3)
    model = _fresh_spp_model(params, batch_norm_decay=0.99)
    trainer = training.Trainer(model, config_optimizer('lamb', 1e-3), ema_decay=0.999)
    with y3.variable_scope('yolov3'):
        losses = [float(trainer.step(x, yts)[0]) for _ in range(3)]
    assert np.isfinite(losses).all()
    ratios = trainer.trust_ratios()
    assert len(ratios) == 225 and all(np.isfinite(v) and v > 0 for v in ratios.values())
    variables = y3.global_variables(scope='yolov3')
    path = Saver(variables).save(str(tmp_path / 'spp'), optimizer=trainer.opt, global_step=3, averages=trainer)
    stored = np.load(path)
    shifted = 'yolov3/yolov3_head/Conv_23/weights'
    assert shifted + EMA_SUFFIX in stored.files and 'yolov3/yolov3_head/Conv_3/weights' + EMA_SUFFIX in stored.files
    assert stored['yolov3/yolov3_head/Conv_3/weights'].shape == (1, 1, 2048, 512)
    assert sum(1 for k in stored.files if k.endswith(EMA_SUFFIX)) == 225
    before = {v.op_name: v.numpy().copy() for v in variables}
    averages = {k: t.cpu().numpy().copy() for k, t in trainer.ema_tensors().items()}
    # a fresh SPP model restores it by name, averages included
    model2 = _fresh_spp_model(sc.spp_params(80, seed=3), batch_norm_decay=0.99)
    trainer2 = training.Trainer(model2, config_optimizer('lamb', 1e-3), ema_decay=0.999)
    variables2 = y3.global_variables(scope='yolov3')
    assert Saver(variables2).restore(path, optimizer=trainer2.opt, averages=trainer2) == 3.0
    for v in variables2:
        np.testing.assert_array_equal(v.numpy(), before[v.op_name], err_msg=v.op_name)
    with y3.variable_scope('yolov3'):
        assert np.isfinite(float(trainer2.step(x, yts)[0]))
    assert set(trainer2.ema_tensors()) == set(averages)
    # a default-architecture model refuses the file at the first variable whose shape differs, by name
    from oracle import yolo_ref
    _fresh_spp_model(yolo_ref.synthetic_params(80, seed=3), spp=False)
    with pytest.raises(ValueError) as err:
        Saver(y3.global_variables(scope='yolov3')).restore(path)
    assert 'yolov3/yolov3_head/Conv_3/weights' in str(err.value)
