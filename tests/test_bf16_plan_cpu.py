"""The guard of tests/test_bf16_plan_gpu.py's per-launch gate, on the CPU with the oracle alone (no device library): the gate
passes an honest bf16 kernel on the real net's operands, and fails each wrong kernel a plan can hide.

Operands: yolo_ref.forward(..., return_trace=True) of the synthetic net at (1,32,64) and (3,96,64) (bf16_plan_cases.WALK[1],
[2]; the /32 maps are 1x2 and 3x2), five layers' real inputs rounded to bf16:
  53  the /32 3x3 512 -> 1024                                   54  the 1x1 1024 -> 512 behind it
  60  the 1x1 768 -> 256 on concat([upsample(layer 59), route 2])
   3  the first residual block's 3x3 32 -> 64 with its shortcut 58  the detection conv 1024 -> 255 (fp32 out, bias, linear)
The kernel's emulation: torch's fp32 convolution of the rounded operands, fp32 scale / shift / LeakyReLU / residual, one
rounding to bf16 (none for the fp32 output).  The reference and the gate: bf16_plan_cases (ref_conv in fp64; 2^-8 |want| +
2e-3 for a bf16 output, 1e-4 |want| + 2e-3 for an fp32 one).

Recorded (elements outside the gate / elements; this file asserts only that the honest count is 0 and every other > 0):
                                                                                     (1,32,64)        (3,96,64)
  the honest emulation, each of the five layers                                      0 misses         0 misses
  one input channel of one tap dropped (layer 53, centre tap, channel 7)           1773 / 2048    15950 / 18432
  one input channel dropped (layer 54, channel 7)                                   905 / 1024     7125 / 9216
  the two concat halves exchanged (layer 60)                                       2040 / 2048    18354 / 18432
  the residual omitted (layer 3)                                                  32326 / 32768  290746 / 294912
  the residual taken one pixel to the right (layer 3)                             29286 / 32768  263156 / 294912
  the top padding row of the 1-pixel-high map read as the centre row (layer 53)    2025 / 2048    (3 rows: no case)
  scale / shift of channel c applied to c + 1 in the last column group, channels
  248..255 of the 255 -> 256 padded detection conv (layer 58)                        12 / 510       108 / 4590
(the last: the six channels that take a neighbour's bias, at every pixel - all of what the mutation changes)"""
import numpy as np
import torch
import torch.nn.functional as F

import bf16_plan_cases as pc
from bf16_plan_cases import bf16_round, ref_conv

SIZES = [pc.WALK[1], pc.WALK[2]]
BN_EPS = 1e-5

_CASES = {}


def _cases(size):
    """per layer of the five: dict(x [, up, resid], w, scale, shift, k, act, kind) of bf16-rounded fp32 arrays"""
    if size in _CASES:
        return _CASES[size]
    from oracle import yolo_ref
    pc.cap_threads()
    n, h, w = size
    params = yolo_ref.synthetic_params(80, seed=1)
    _, trace = yolo_ref.forward(params, pc.images(SIZES.index(size) + 1, n, h, w), return_trace=True)
    assert len(trace) == 75
    out = [t for _, t in trace]
    name = lambda i: trace[i][0]

    def fold(i):
        g, b, m, v = (params['%s/BatchNorm/%s' % (name(i), s)] for s in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
        scale = (g / np.sqrt(v + np.float32(BN_EPS))).astype(np.float32)
        return scale, (b - m * scale).astype(np.float32)

    route2 = out[26]                        # the stride-2 conv to 512 channels, then eight residual blocks
    for j in range(8):
        route2 = out[28 + 2 * j] + route2
    wq = lambda i: bf16_round(params[name(i) + '/weights'])
    cases = {}
    for i, extra in ((53, {}), (54, {}), (60, dict(up=bf16_round(out[59]), x=bf16_round(route2))), (3, dict(resid=bf16_round(out[1])))):
        scale, shift = fold(i)
        c = dict(x=bf16_round(out[i - 1]), w=wq(i), scale=scale, shift=shift, k=wq(i).shape[0], act=True, kind='bf16')
        c.update(extra)
        cases[i] = c
    cases[58] = dict(x=bf16_round(out[57]), w=wq(58), scale=np.ones(255, np.float32), shift=params[name(58) + '/biases'].astype(np.float32),
                     k=1, act=False, kind='f32')
    assert cases[53]['w'].shape == (3, 3, 512, 1024) and cases[54]['w'].shape == (1, 1, 1024, 512)
    assert cases[60]['w'].shape == (1, 1, 768, 256) and cases[60]['up'].shape[3] == 256 and cases[60]['x'].shape[3] == 512
    assert cases[3]['w'].shape == (3, 3, 32, 64) and cases[58]['w'].shape == (1, 1, 1024, 255)
    assert cases[53]['x'].shape[1:3] == (h // 32, w // 32)
    _CASES[size] = cases
    return cases


def _want(c):
    xin = pc.upcat(c['up'], c['x']) if 'up' in c else c['x']
    return ref_conv(xin, c['w'], c['scale'], c['shift'], c['k'], 1, c['act'], c.get('resid'))


def _emulate(c, xin=None, w=None, scale=None, shift=None, resid='own', pad=None):
    """the kernel on the CPU: fp32 accumulation, fp32 epilogue, one rounding.  pad: (the NHWC input padded by hand, torch padding)"""
    if xin is None:
        xin = pc.upcat(c['up'], c['x']) if 'up' in c else c['x']
    w = c['w'] if w is None else w
    scale = c['scale'] if scale is None else scale
    shift = c['shift'] if shift is None else shift
    resid = c.get('resid') if isinstance(resid, str) else resid
    padding = c['k'] // 2
    if pad is not None:
        xin, padding = pad
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(xin)).permute(0, 3, 1, 2), torch.from_numpy(w).permute(3, 2, 0, 1).contiguous(),
                 padding=padding)
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1)
    if c['act']:
        y = torch.where(y > 0, y, 0.1 * y)
    y = y.permute(0, 2, 3, 1)
    if resid is not None:
        y = y + torch.from_numpy(resid)
    y = y.contiguous().numpy()
    return y if c['kind'] == 'f32' else bf16_round(y)


def _mutations(cases):
    """name -> (layer, the wrong kernel's output)"""
    out = {}
    c = cases[53]
    w = c['w'].copy()
    w[1, 1, 7, :] = 0
    out['one input channel of one tap dropped (3x3 512->1024, centre tap, channel 7)'] = (53, _emulate(c, w=w))
    c = cases[54]
    w = c['w'].copy()
    w[0, 0, 7, :] = 0
    out['one input channel dropped (1x1 1024->512, channel 7)'] = (54, _emulate(c, w=w))
    c = cases[60]
    up2 = np.repeat(np.repeat(c['up'], 2, 1), 2, 2)
    out['the two concat halves exchanged (768->256)'] = (60, _emulate(c, xin=np.concatenate([c['x'], up2], axis=3)))
    c = cases[3]
    out['the residual omitted (first block)'] = (3, _emulate(c, resid=None))
    r = c['resid']
    out['the residual taken one pixel to the right (first block)'] = (3, _emulate(c, resid=np.concatenate([r[:, :, 1:], r[:, :, -1:]], axis=2)))
    c = cases[53]
    if c['x'].shape[1] == 1:
        x = c['x']
        by_hand = np.concatenate([x, x, np.zeros_like(x)], axis=1)          # rows -1, 0, 1: the top padding row reads row 0
        out['the top padding row of the 1-pixel-high map read as the centre row (3x3 512->1024)'] = \
            (53, _emulate(c, pad=(by_hand, (0, 1))))
    c = cases[58]
    scale, shift = c['scale'].copy(), c['shift'].copy()
    scale[249:255], shift[249:255] = c['scale'][248:254], c['shift'][248:254]      # the last 8 columns 248..255 (255 is padding)
    out['scale / shift of channel c applied to c + 1 in the last column group of the detection conv'] = (58, _emulate(c, scale=scale, shift=shift))
    return out


def measure():
    """every count this file's docstring records: [(size, what, misses, elements)]"""
    rows = []
    for size in SIZES:
        cases = _cases(size)
        wants = {i: _want(c) for i, c in cases.items()}
        for i, c in sorted(cases.items()):
            rows.append((size, 'honest layer %d' % i, int(pc.misses(_emulate(c), wants[i], c['kind']).sum()), wants[i].size))
        for what, (i, got) in _mutations(cases).items():
            rows.append((size, what, int(pc.misses(got, wants[i], cases[i]['kind']).sum()), wants[i].size))
    return rows


def test_the_gate_passes_the_honest_kernel_and_fails_every_mutation():
    rows = measure()
    for size, what, miss, total in rows:
        print('%s %s: %d / %d' % (size, what, miss, total))
    seen = set()
    for size, what, miss, total in rows:
        if what.startswith('honest'):
            assert miss == 0, (size, what, miss)
        else:
            assert miss > 0, 'the gate is too loose to see: %s at %s' % (what, size)
            seen.add(what)
    assert len(seen) == 7, sorted(seen)


def test_the_gate_is_the_one_test_bf16_gpu_states():
    want = np.array([-50.0, 0.0, 0.3, 7.0])
    np.testing.assert_array_equal(pc.tolerance(want, 'bf16'), 2.0 ** -8 * np.abs(want) + 2e-3)
    np.testing.assert_array_equal(pc.tolerance(want, 'f32'), 1e-4 * np.abs(want) + 2e-3)
    np.testing.assert_array_equal(pc.tolerance(want, 'fused'), 2.0 ** -7 * np.abs(want) + 2e-2)
    got = want + np.array([0.19, 0.0021, np.nan, -0.02])
    assert pc.misses(got, want, 'bf16').tolist() == [False, True, True, False]
    x = np.arange(2 * 2 * 3 * 8, dtype=np.float32).reshape(2, 2, 3, 8)
    pooled = pc.spp_concat(x)
    assert pooled.shape == (2, 2, 3, 32) and np.array_equal(pooled[..., 24:], x)
    assert np.array_equal(pooled[..., :8], np.broadcast_to(x.max(axis=(1, 2), keepdims=True), x.shape))
    up = np.arange(4, dtype=np.float32).reshape(1, 1, 2, 2)
    cat = pc.upcat(up, np.zeros((1, 2, 4, 1), np.float32))
    assert cat.shape == (1, 2, 4, 3) and cat[0, 1, 3, :2].tolist() == [2.0, 3.0] and cat[0, 0, 1, :2].tolist() == [0.0, 1.0]
