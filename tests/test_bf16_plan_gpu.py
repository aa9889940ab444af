"""GPU tests that hold the bf16 inference plan (compute_dtype = 'bf16', net dtype 1) to its own kernels and to fp64, layer
by layer, in both architectures (helpers: tests/bf16_plan_cases.py).

  1. y3_net_forward equals its op-by-op composition through the per-op entries, BIT FOR BIT, while ONE net handle walks
     through the six input sizes of bf16_plan_cases.WALK on a workspace full of 0xFF bytes (a NaN in bf16 and in fp32) and
     into feature maps full of NaN: a residual read from a buffer the arena has handed on, a stale route, offset or pool
     offset of the size before, a concat whose halves are swapped, a fused launch that mishandles a ragged tile all change
     bits.  The same forward into a fresh workspace of exactly y3_net_workspace_bytes and model.forward give the same bits.
  2. every launch of that composition against an fp64 convolution of the launch's own inputs as they are on the device, at
     the tolerances tests/test_bf16_gpu.py states (one bf16 ulp; the two fused pairs two).  The composition is the plan
     (1.), so this is one-ulp parity of every launch of the real net, on the real net's activations and weights.

The walk's sizes run tiles E, f, o, s, x (asserted).  D, d and e need launches of the size of batch 16 at 608 and stay with
test_bf16_gpu.py::test_bf16_conv_matches_fp64_on_rounded_operands."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_plan_cases as pc

pytestmark = pytest.mark.gpu

_COMPOSED = {}      # (arch, n, h, w) -> (tensors, maps, launches, layer parameters): computed once, left unchanged.  The
                    # parameters of an architecture are the same in every model of this file (seed 1), so is the composition.


def _model(arch, request):
    """the session's gpu_model, or a fresh SPP model under isolated_graph as tests/test_spp_gpu.py builds it"""
    if arch == 'default':
        return request.getfixturevalue('gpu_model')[0]
    import spp_cases as sc
    from test_spp_gpu import _fresh_spp_model
    request.getfixturevalue('isolated_graph')
    return _fresh_spp_model(sc.spp_params(80, seed=1))


def _composed(model, arch, step):
    """the composition at WALK[step]; under the model's graph and variable scope, compute_dtype 'bf16'"""
    n, h, w = pc.WALK[step]
    key = (arch, n, h, w)
    if key not in _COMPOSED:
        fw, _lib, L, ctx, dev = pc.env()
        x = torch.from_numpy(pc.images(step, n, h, w)).to(dev)
        tens, maps, launches = pc.compose_bf16(model, x, pc.ARCHS[arch])
        _COMPOSED[key] = (tens, maps, launches, pc.layer_params(model, pc.topology(model.class_num, pc.ARCHS[arch])))
    return _COMPOSED[key]


def _forward(L, _lib, fw, net, x, ws, fms):
    n, h, w, _ = x.shape
    ws.fill_(0xFF)
    for f in fms:
        f.fill_(float('nan'))
    _lib.check(L.y3_net_forward(net, fw.ptr(x), n, h, w, fw.ptr(ws), ctypes.c_size_t(ws.numel()), *[fw.ptr(f) for f in fms]))


def walk_the_plan(model, arch, fused=(pc.FUSED,), tiles=pc.TILES):
    """The body of the walk.  fused: the reports y3_net_layer_fused may give for layers 0-3, at every size; tiles: the set of
    letters y3_conv_bf16_tile must give over the walk's layers (None: not asserted - a build of the library that routes
    otherwise; the composer follows whatever is reported)."""
    import yolov3_tensorflow_amd as y3
    fw, _lib, L, ctx, dev = pc.env()
    topo = pc.topology(model.class_num, pc.ARCHS[arch])
    det = 3 * (5 + model.class_num)
    with pc.TableNet(model.class_num, pc.ARCHS[arch]) as tn:      # (sized on another handle: the walked one plans in walk order only)
        big = max(tn.workspace_bytes(*s) for s in pc.WALK)
    assert any(h // 32 == 1 for _, h, _ in pc.WALK)
    seen = set()
    previous = model.compute_dtype
    model.compute_dtype = 'bf16'
    try:
        with y3.variable_scope('yolov3'):
            net = model._get_net(dev)['handle']
            ws = torch.empty(big, dtype=torch.uint8, device=dev)
            for step, (n, h, w) in enumerate(pc.WALK):
                x = torch.from_numpy(pc.images(step, n, h, w)).to(dev)
                fms = [torch.empty((n, h // s, w // s, det), device=dev) for s in (32, 16, 8)]
                _forward(L, _lib, fw, net, x, ws, fms)
                flags = [L.y3_net_layer_fused(net, i, n, h, w) for i in range(len(topo.layers))]
                assert flags[:4] in [list(f) for f in fused], ((n, h, w), flags[:4])
                assert not any(flags[4:]), flags
                seen |= set(pc.tile_letters(topo, n, h, w))
                _, composed, _, _ = _composed(model, arch, step)
                need = L.y3_net_workspace_bytes(net, n, h, w)
                assert 0 < need <= big
                fresh_ws = torch.empty(need, dtype=torch.uint8, device=dev)
                again = [torch.empty_like(f) for f in fms]
                _forward(L, _lib, fw, net, x, fresh_ws, again)
                through_model = model.forward(x, False)
                torch.cuda.synchronize()
                fw.check_context()
                for j, (a, b, c, d) in enumerate(zip(fms, composed, again, through_model)):
                    where = 'feature map %d at %s (%s)' % (j + 1, (n, h, w), arch)
                    assert bool(torch.isfinite(a).all()), where + ': not finite'
                    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
                    if not torch.equal(a, b):
                        diff = (a != b)
                        raise AssertionError('%s: plan != composition at %d of %d elements, first at %s; max |d| %.3e' % (
                            where, int(diff.sum()), diff.numel(), tuple(int(v) for v in diff.nonzero()[0]), float((a - b).abs().max())))
                    assert torch.equal(a, c), where + ': another result in a fresh workspace of exactly y3_net_workspace_bytes'
                    assert torch.equal(a, d), where + ': model.forward gives other bits'
    finally:
        model.compute_dtype = previous
    print('%s: tiles over the walk: %s; fused flags of layers 0-3: %s' % (arch, ''.join(sorted(seen)), flags[:4]))
    if tiles is not None:
        assert seen == set(tiles), sorted(seen)


@pytest.mark.parametrize('arch', sorted(pc.ARCHS))
def test_plan_equals_its_composition_bit_for_bit_over_the_size_walk(arch, request):
    walk_the_plan(_model(arch, request), arch)


def test_plan_equals_its_composition_whatever_the_library_routes(gpu_model):
    """The walk of the default architecture, the first block fused or not and no tile letters asserted: the case that
    tests/test_conv_variants_gpu.py runs on the experiments build with every 1x1 conv on the ring kernel, where
    y3_conv_bf16_resblock64_takes refuses the first residual block (flags 1, 2, 0, 0) and the 1x1 kernels are packed otherwise."""
    walk_the_plan(gpu_model[0], 'default', fused=(pc.FUSED, [1, 2, 0, 0]), tiles=None)


@pytest.mark.parametrize('step', range(len(pc.WALK)), ids=['%dx%dx%d' % s for s in pc.WALK])
@pytest.mark.parametrize('arch', sorted(pc.ARCHS))
def test_every_launch_matches_fp64_on_its_own_inputs(arch, step, request):
    """Each launch of the composition (= the plan, bit for bit: the walk above) against ref_conv in fp64 on the launch's own
    device inputs.  The synthetic net's activations have rms 0.15-7 and max about 50, so the absolute terms of the gates
    stay small against the signal."""
    import yolov3_tensorflow_amd as y3
    pc.cap_threads()
    n, h, w = pc.WALK[step]
    key = (arch, n, h, w)
    if key not in _COMPOSED:
        model = _model(arch, request)
        previous, model.compute_dtype = model.compute_dtype, 'bf16'
        try:
            with y3.variable_scope('yolov3'):
                _composed(model, arch, step)
        finally:
            model.compute_dtype = previous
    tens, maps, launches, P = _COMPOSED[key]
    topo = pc.topology(80, pc.ARCHS[arch])
    assert sum(len(l['layers']) for l in launches) == len(topo.layers)
    failures, worst = [], {}
    for launch in launches:
        want, kind = pc.launch_reference(launch, tens, P, topo)
        got = tens[launch['dst']].float().cpu().numpy()
        assert got.shape == want.shape, (launch['layers'], got.shape, want.shape)
        ratio = float((np.abs(got - want) / pc.tolerance(want, kind)).max()) if np.isfinite(got).all() else float('inf')
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        if pc.misses(got, want, kind).any():
            failures.append(pc.describe_miss(launch, topo, got, want, kind))
    print('%s %s: %d launches; largest |d| / tolerance per gate: %s' % (
        arch, (n, h, w), len(launches), ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))
    assert not failures, '\n'.join(failures)
