"""The layer-wise update rules without a GPU (include/yolo355.h, "Layer-wise update rules"; kernels:
test_layerwise_update_gpu.py): the rules pinned by hand, their restatement, the Python surface, the checkpoint keys, the strip
tool, the train.py options, and what float32 arithmetic costs against the fp64 rule."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import layerwise_cases as LC


def _two(w, g, s0, s1, wd, flags=0):
    f = lambda a: None if a is None else np.array(a, np.float32)
    return dict(w=f(w), g=f(g), s0=f(s0), s1=f(s1), wd=wd, flags=flags)


# exact small numbers: betas of 0.5 and 0.75, a 3-4-5 gradient and weight, no rounding anywhere but the roots
_HP = dict(grad_scale=1.0, clip_norm=100.0, lr=0.5, lr_t=0.25, momentum=0.5, beta1=0.5, beta2=0.75, eps=0.0, bias1=2.0, bias2=4.0,
           trust=0.5, ema_step=0.0)


def test_adamw_by_hand():
    """w = (3, 4), g = (6, 8), m = (2, 0), v = (4, 16), lambda = 0.5.  G = 10 (no clip).
    m = 0.5 m + 0.5 g = (4, 4); v = 0.75 v + 0.25 g^2 = (12, 28); w - lr_t m / sqrt(v) - lr lambda w."""
    o = LC.evaluate('adamw', _two([3, 4], [6, 8], [2, 0], [4, 16], 0.5), _HP)
    np.testing.assert_array_equal(o['s0'], [4.0, 4.0])
    np.testing.assert_array_equal(o['s1'], [12.0, 28.0])
    np.testing.assert_array_equal(o['g'], [6.0, 8.0])
    np.testing.assert_allclose(o['w'], [3 - 0.25 * 4 / np.sqrt(12.0) - 0.75, 4 - 0.25 * 4 / np.sqrt(28.0) - 1.0], rtol=1e-15)
    assert o['ratio'] == 1.0
    # the clip: grad_scale 50 makes G = 500, c = 0.2, gh = (60, 80)
    o = LC.evaluate('adamw', _two([3, 4], [6, 8], [2, 0], [4, 16], 0.5), dict(_HP, grad_scale=50.0))
    np.testing.assert_allclose(o['g'], [60.0, 80.0], rtol=1e-15)


def test_lars_by_hand():
    """w = (3, 4): W = 5; g = (6, 8): Gh = 10; lambda = 0.5: ratio = 0.5 * 5 / (10 + 2.5) = 0.2.
    u = g + 0.5 w = (7.5, 10); acc = 0.5 (2, -2) + 0.2 u = (2.5, 1); w - 0.5 acc = (1.75, 3.5)."""
    t = _two([3, 4], [6, 8], [2, -2], None, 0.5)
    o = LC.evaluate('lars', t, _HP)
    assert o['ratio'] == pytest.approx(0.2, rel=1e-15)
    np.testing.assert_allclose(o['s0'], [2.5, 1.0], rtol=1e-15)
    np.testing.assert_allclose(o['w'], [1.75, 3.5], rtol=1e-15)
    np.testing.assert_array_equal(o['g'], [6.0, 8.0])
    # NO_ADAPT, a zero weight and a zero gradient: ratio 1, and the plain momentum rule with lambda after the clip
    for t1 in (dict(t, flags=LC.NO_ADAPT), dict(t, w=np.zeros(2, np.float32)), dict(t, g=np.zeros(2, np.float32))):
        o = LC.evaluate('lars', t1, _HP)
        assert o['ratio'] == 1.0
        u = t1['g'].astype(np.float64) + 0.5 * t1['w']
        np.testing.assert_array_equal(o['s0'], 0.5 * t['s0'] + u)
        np.testing.assert_array_equal(o['w'], t1['w'] - 0.5 * o['s0'])


def test_lamb_by_hand():
    """w = (3, 4): W = 5; g = (6, 8), m0 = (2, 0), v0 = (4, 16): m = (4, 4), v = (12, 28) as for AdamW;
    r = 2 m / sqrt(4 v) + 0.5 w = (8 / sqrt(48) + 1.5, 8 / sqrt(112) + 2); ratio = 5 / |r|; w - 0.5 ratio r."""
    t = _two([3, 4], [6, 8], [2, 0], [4, 16], 0.5)
    o = LC.evaluate('lamb', t, _HP)
    r = np.array([8 / np.sqrt(48.0) + 1.5, 8 / np.sqrt(112.0) + 2.0])
    np.testing.assert_allclose(o['g'], r, rtol=1e-15)
    assert o['ratio'] == pytest.approx(5.0 / np.sqrt((r * r).sum()), rel=1e-15)
    np.testing.assert_allclose(o['w'], np.array([3.0, 4.0]) - 0.5 * o['ratio'] * r, rtol=1e-15)
    np.testing.assert_array_equal(o['s0'], [4.0, 4.0])
    np.testing.assert_array_equal(o['s1'], [12.0, 28.0])
    o = LC.evaluate('lamb', dict(t, flags=LC.NO_ADAPT), _HP)
    assert o['ratio'] == 1.0
    np.testing.assert_allclose(o['w'], np.array([3.0, 4.0]) - 0.5 * r, rtol=1e-15)
    # g = 0, m = 0, lambda = 0: the direction is zero, the ratio 1 and w stays
    o = LC.evaluate('lamb', _two([3, 4], [0, 0], [0, 0], [4, 16], 0.0), _HP)
    assert o['ratio'] == 1.0
    np.testing.assert_array_equal(o['w'], [3.0, 4.0])
    np.testing.assert_array_equal(o['g'], [0.0, 0.0])


@pytest.mark.parametrize('kind', LC.KINDS)
def test_restatement_is_the_rule_and_every_perturbed_form_is_far(kind):
    """restated(perturb=None) is evaluate, bit for bit (fp64), on the shared inputs: a guard then differs from the expectation
    by the named perturbation alone.  And fp64 against fp64, every perturbed form is more than 100 tolerances from the rule on
    some output (printed), so the GPU test's guards can bite."""
    hp = LC.hyper(kind)
    want = LC.expected(kind)
    for t, e in zip(LC.inputs(kind), want):
        o = LC.restated(kind, t, hp)
        for k in LC.OUTPUTS:
            assert (o[k] is None) == (e[k] is None)
            if e[k] is not None:
                np.testing.assert_array_equal(o[k], e[k])
    for perturb in LC.GUARDS[kind]:
        d = LC.distance(LC.expected(kind, perturb), want)
        print('%s / %s: tolerances away: %s' % (kind, perturb, ', '.join('%s %.0f' % (k, v / LC.TOL) for k, v in d.items())))
        assert max(d.values()) > LC.GUARD * LC.TOL, (perturb, d)


def test_shared_inputs_are_what_the_header_of_the_cases_says():
    for kind in LC.KINDS:
        ins, want = LC.inputs(kind), LC.expected(kind)
        assert [t['w'].size for t in ins] == list(LC.SIZES)
        assert not ins[LC.ZERO_W]['w'].any() and not ins[LC.ZERO_G]['g'].any()
        assert want[LC.ZERO_W]['ratio'] == 1.0 and want[LC.ZERO_G]['ratio'] == 1.0
        assert sum(1 for t in ins if t['flags'] & LC.NO_ADAPT) == 2 and all(e['ratio'] == 1.0 for t, e in zip(ins, want) if t['flags'])
        assert {t['wd'] for t in ins} == {0.0, LC.F32(5e-2)}
        for i, t in enumerate(ins):
            norm = LC.hyper(kind)['grad_scale'] * float(np.sqrt((t['g'].astype(np.float64) ** 2).sum()))
            assert (norm > 120.0) if LC.NORM[i] > 100.0 else (norm < 80.0), (i, norm)       # clipped / not clipped
            assert t['s0'].any() or i == LC.ZERO_G
        if kind != 'adamw':     # the adapted tensors' ratios are far from 1
            assert all(abs(e['ratio'] - 1.0) > 0.2 for i, (t, e) in enumerate(zip(ins, want))
                       if not t['flags'] and i not in (LC.ZERO_W, LC.ZERO_G))


@pytest.mark.parametrize('kind', LC.KINDS)
def test_float32_evaluation_against_fp64(kind):
    """What fp32 arithmetic alone costs: evaluate(dtype=float32) against fp64 on the shared inputs, worst error per output as a
    fraction of the tensor's max |expected| (printed).  The GPU test's tolerance of 2e-6 stands where this figure is at most
    a eighth of it, which is asserted here (measured: 0.6e-7 to 1.7e-7)."""
    hp = LC.hyper(kind)
    got = [LC.evaluate(kind, t, hp, np.float32) for t in LC.inputs(kind)]
    for o in got:
        assert all(o[k] is None or np.asarray(o[k]).dtype == np.float32 for k in LC.OUTPUTS)
    worst = LC.distance(got, LC.expected(kind))
    print('float32 numpy %s: worst error / max|expected|: %s' % (kind, LC.fmt(worst)))
    assert max(worst.values()) <= LC.TOL / 8, worst


def test_optimizer_and_config_optimizer_know_the_names():
    from yolov3_tensorflow_amd import training, _lib
    from yolov3_tensorflow_amd.utils import misc_utils
    assert training.Optimizer.KINDS == ('sgd', 'momentum', 'adam', 'rmsprop', 'adamw', 'lars', 'lamb')
    for kind in LC.KINDS:
        assert training.Optimizer.KINDS.index(kind) == LC.KIND_ID[kind]
    assert (_lib.Y3_OPT_ADAMW, _lib.Y3_OPT_LARS, _lib.Y3_OPT_LAMB, _lib.Y3_PARAM_NO_ADAPT) == (4, 5, 6, LC.NO_ADAPT)
    assert ctypes.sizeof(_lib.LayerwiseHp) == 48 and [n for n, _ in _lib.LayerwiseHp._fields_] == list(LC.HP_FIELDS)
    assert training.Optimizer('adamw', 1e-3).epsilon == 1e-8 and training.Optimizer('lamb', 1e-3).epsilon == 1e-6
    assert training.Optimizer('lars', 1e-3).trust == 0.001 and training.Optimizer('lars', 1e-3, trust=0.02).trust == 0.02
    assert training.Optimizer('adam', 1e-3).epsilon == 1e-8 and training.Optimizer('rmsprop', 1e-3).epsilon == 1e-10
    for kind in LC.KINDS:
        opt = misc_utils.config_optimizer(kind, 1e-3, momentum=0.7, trust=0.05)
        assert opt.kind == kind and opt.step == 0 and opt.slots == {}
        assert (opt.momentum, opt.trust) == ((0.7, 0.05) if kind == 'lars' else (0.9, 0.001))
        import test_ema_cpu as TE
        s0, s1 = opt._slots_for(TE.CpuVar('yolov3/a/weights', np.ones((1, 1, 3, 4))))
        assert not s0.any() and (s1 is None if kind == 'lars' else not s1.any())
    with pytest.raises(ValueError):
        misc_utils.config_optimizer('lion', 1e-3)


def test_slot_names_round_trip_through_saver(tmp_path):
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils import misc_utils
    import test_ema_cpu as TE
    names = dict(adamw=('AdamW', 'AdamW_1'), lars=('LARS',), lamb=('LAMB', 'LAMB_1'))
    for kind in LC.KINDS:
        assert misc_utils._SLOT_NAMES[kind] == names[kind]
        src = TE._variables()
        opt = training.Optimizer(kind, 1e-3)
        r = np.random.RandomState(3)
        for v in src:
            opt.slots[v.op_name] = tuple(torch.tensor(r.standard_normal(v.shape).astype(np.float32)) if j < LC.SLOTS[kind] else None
                                         for j in range(2))
        opt.step = 11
        path = misc_utils.Saver(src).save(str(tmp_path / kind), optimizer=opt, global_step=11.0)
        stored = np.load(path)
        assert sorted(stored.files) == sorted([v.op_name for v in src] + [v.op_name + '/' + s for v in src for s in names[kind]]
                                              + ['optimizer/step', 'global_step'])
        back = training.Optimizer(kind, 1e-3)
        assert misc_utils.Saver(TE._variables(seed=1)).restore(path, optimizer=back) == 11.0
        assert back.step == 11 and sorted(back.slots) == sorted(opt.slots)
        for k, slots in opt.slots.items():
            for a, b in zip(slots, back.slots[k]):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        # another kind's slots are not taken for this one's
        other = training.Optimizer('momentum', 1e-3)
        misc_utils.Saver(TE._variables()).restore(path, optimizer=other)
        assert other.slots == {}


def test_strip_tool_drops_the_new_slots(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'misc'))
    import remove_optimizers_params_in_ckpt as rm
    r = np.random.RandomState(0)
    var = 'yolov3/darknet53_body/Conv/weights'
    arrays = {var: r.rand(3, 3, 3, 8).astype(np.float32), 'optimizer/step': np.int64(2), 'global_step': np.float64(2)}
    for s in ('AdamW', 'AdamW_1', 'LARS', 'LAMB', 'LAMB_1'):
        arrays[var + '/' + s] = r.rand(3, 3, 3, 8).astype(np.float32)
    src = str(tmp_path / 'full.npz')
    np.savez(src, **arrays)
    keep, drop = rm.main([src, '--output', str(tmp_path / 'small.npz')])
    assert keep == [var] and sorted(drop) == sorted(k for k in arrays if k != var)
    np.testing.assert_array_equal(np.load(str(tmp_path / 'small.npz'))[var], arrays[var])


def test_train_parser_knows_the_options():
    sys.path.insert(0, ROOT)
    import train as train_script
    parser = train_script.build_parser()
    assert parser.parse_args([]).optimizer_name == 'momentum' and parser.parse_args([]).lars_trust == 0.001
    for kind in LC.KINDS:
        assert parser.parse_args(['--optimizer_name', kind]).optimizer_name == kind
    assert parser.parse_args(['--optimizer_name', 'lars', '--lars_trust', '0.02']).lars_trust == 0.02
    text = parser.format_help()
    assert 'adamw | lars | lamb' in text and 'decoupled' in text


def test_the_library_exports_the_entry_points_and_sizes_the_scratch():
    """host-only: the symbols load without a GPU; the scratch holds descriptors, two partials per chunk, four statistics, a
    shadow pointer and a flag word per tensor, and is 0 for no tensors"""
    from yolov3_tensorflow_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert hasattr(L, 'y3_layerwise_update_multi')
    arr = (_lib.ParamDesc * 2)()
    arr[0] = _lib.ParamDesc(None, None, None, None, 7, 0.0, 0)
    arr[1] = _lib.ParamDesc(None, None, None, None, 8193, 0.0, 0)
    nb = L.y3_layerwise_update_multi_scratch_bytes(arr, 2)
    assert nb >= 2 * 48 + 3 * 2 * 4 + 2 * 4 * 4 + 2 * (8 + 4) and nb > L.y3_clip_update_multi_ema_scratch_bytes(arr, 2)
    assert L.y3_layerwise_update_multi_scratch_bytes(arr, 0) == 0 and L.y3_layerwise_update_multi_scratch_bytes(None, 2) == 0
    # a refusal needs no device: the arguments are checked first
    hp = LC.hp_struct(LC.hyper('lamb'))
    dummy = ctypes.c_void_p(256)
    assert L.y3_layerwise_update_multi(None, 6, arr, 2, ctypes.byref(hp), None, None, dummy, ctypes.c_size_t(nb)) == _lib.Y3_EINVAL
    assert L.y3_layerwise_update_multi(dummy, 3, arr, 2, ctypes.byref(hp), None, None, dummy, ctypes.c_size_t(nb)) == _lib.Y3_EINVAL
    assert L.y3_layerwise_update_multi(dummy, 6, arr, 2, None, None, None, dummy, ctypes.c_size_t(nb)) == _lib.Y3_EINVAL


def test_per_tensor_experiment_hook_refuses_the_new_kinds(monkeypatch):
    """Y3_TRAIN_PER_TENSOR_UPDATE=1 (one y3_clip_update per variable) knows the four old kinds: a clear error before anything
    is touched"""
    from yolov3_tensorflow_amd import training
    monkeypatch.setenv('Y3_TRAIN_PER_TENSOR_UPDATE', '1')
    for kind in LC.KINDS:
        tr = training.Trainer(None, training.Optimizer(kind, 1e-3))
        with pytest.raises(RuntimeError, match='Y3_TRAIN_PER_TENSOR_UPDATE'):
            tr.apply_gradients()
        assert tr.opt.step == 0 and tr.global_step == 0.0
