"""The weight moving average without a GPU: the decay schedule, the scratch queries, the checkpoint keys, the strip tool and
the new symbols (include/yolo355.h, "Weight moving average"; kernels: test_ema_gpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import ema_cases as E


class CpuVar(object):
    """a variable on CPU tensors with the interface Saver and Trainer use"""
    trainable = True

    def __init__(self, name, value):
        self.op_name, self.tensor, self.version = name, torch.tensor(np.asarray(value, np.float32)), 0
        self.shape = tuple(self.tensor.shape)

    def assign(self, value, validate_shape=True):
        value = np.asarray(value, np.float32)
        if validate_shape and tuple(value.shape) != self.shape:
            raise ValueError('shape')
        self.tensor = torch.tensor(value)
        self.touch()

    def touch(self):
        self.version += 1

    def numpy(self):
        return self.tensor.numpy()


def _trainer(variables, averaged_names, **kw):
    """a Trainer whose update order is `averaged_names` (what the first step would derive from update_vars)"""
    from yolov3_tensorflow_amd import training
    tr = training.Trainer(None, training.Optimizer('sgd', 1e-3), **kw)
    tr.order = [v for v in variables if v.op_name in averaged_names]
    tr._alloc_ema()
    return tr


def _variables(seed=0):
    r = np.random.RandomState(seed)
    shapes = (('yolov3/a/weights', (1, 1, 3, 4)), ('yolov3/a/biases', (4,)), ('yolov3/b/weights', (1, 1, 4, 5)),
              ('yolov3/b/BatchNorm/gamma', (5,)))
    return [CpuVar(n, r.standard_normal(s)) for n, s in shapes]


def test_schedule_is_the_closed_form_in_double():
    from yolov3_tensorflow_amd import training
    opt = training.Optimizer('sgd', 1e-3)
    tr = training.Trainer(None, opt, ema_decay=0.9998)
    assert tr.ema_step_at(0) == 1.0 - 1.0 / 10.0
    for t in (0, 1, 7, 100, 44989, 44990, 44991, 10 ** 6):
        assert tr.ema_step_at(t) == 1.0 - min(0.9998, (1.0 + t) / (10.0 + t)) == E.step_at(0.9998, t)
        assert tr.ema_step_at(float(t)) == tr.ema_step_at(t)
    # (1 + t) / (10 + t) >= 0.9998 from t = 44990 on: the plain step factor, bit for bit
    assert (1.0 + 44990) / (10.0 + 44990) >= 0.9998 > (1.0 + 44989) / (10.0 + 44989)
    assert tr.ema_step_at(44990) == 1.0 - 0.9998 and tr.ema_step_at(44989) > 1.0 - 0.9998
    flat = training.Trainer(None, opt, ema_decay=0.9998, ema_warmup=False)
    assert flat.ema_step_at(0) == flat.ema_step_at(10 ** 6) == 1.0 - 0.9998
    # what the float the ABI carries keeps of it: the double's nearest float, not 1 - float32(decay) (3e-4 away)
    assert abs(E.f32(1.0 - 0.9998) / 0.0002 - 1.0) < 2.0 ** -24
    assert abs((1.0 - float(np.float32(0.9998))) / 0.0002 - 1.0) > 1e-4
    # off: None and 0 are the same, and there is no schedule to ask for
    for off in (None, 0, 0.0):
        t0 = training.Trainer(None, opt, ema_decay=off)
        assert t0.ema_decay is None and t0.ema_tensors() == {}
        with pytest.raises(RuntimeError):
            t0.ema_step_at(0)
        with t0.averaged():
            pass
    for bad in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            training.Trainer(None, opt, ema_decay=bad)


def _descs(sizes):
    from yolov3_tensorflow_amd import _lib
    arr = (_lib.ParamDesc * len(sizes))()
    for i, n in enumerate(sizes):
        arr[i] = _lib.ParamDesc(None, None, None, None, n, 0.0, 0)
    return arr


def test_scratch_queries():
    """The plain query returns what it returned before the moving average existed (the numbers are the parent commit's:
    [descriptors, 48 bytes each][one float per 8192-element chunk], each rounded to 256, + 4 bytes per tensor + 256); the new
    query adds the shadow pointers behind it."""
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    parent = {E.SIZES: 1060, (300000,): 772, (7, 255, 8192, 8196, 8193, 300000, 18, 1024): 1056, (1,): 772,
              tuple([8192] * 222): 12920}
    for sizes, want in parent.items():
        arr = _descs(sizes)
        plain, ema = L.y3_clip_update_multi_scratch_bytes(arr, len(sizes)), L.y3_clip_update_multi_ema_scratch_bytes(arr, len(sizes))
        assert plain == want, (sizes[:4], plain, want)
        assert ema >= plain + 8 * len(sizes) and ema == (plain + 255) // 256 * 256 + 8 * len(sizes)
    assert L.y3_clip_update_multi_ema_scratch_bytes(None, 3) == 0 and L.y3_clip_update_multi_ema_scratch_bytes(_descs((4,)), 0) == 0


def test_symbols_and_version():
    from yolov3_tensorflow_amd import _lib
    import test_abi
    L = _lib.lib()
    assert L.y3_abi_version() == 5
    declared = test_abi.declared_symbols()
    for name in ('y3_clip_update_multi_ema', 'y3_ema_update', 'y3_clip_update_multi_ema_scratch_bytes'):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(L, name)


def test_argument_checks_need_no_device():
    """Y3_EINVAL with text before anything is launched: a NULL shadow array, an ema_step outside [0, 1] or not finite, a
    misaligned shadow, a shadow equal to or overlapping w, g or a slot.  (Pointers are never dereferenced on these paths; the
    context is a dummy.)"""
    from yolov3_tensorflow_amd import _lib
    L = _lib.lib()
    ctx, cf, n = ctypes.c_void_p(4096), ctypes.c_float, 64
    base = 1 << 20
    w, g, s0, s1, sh = base, base + 4096, base + 8192, base + 12288, base + 16384
    arr = (_lib.ParamDesc * 1)(_lib.ParamDesc(w, g, s0, s1, n, 0.0, 0))
    sb = L.y3_clip_update_multi_ema_scratch_bytes(arr, 1)
    hp = (cf(1.0), cf(100.0), cf(1e-3), cf(0.9), cf(0.9), cf(0.999), cf(1e-8))

    def multi(ema, step, scratch=ctypes.c_void_p(base + 65536), nbytes=sb):
        return L.y3_clip_update_multi_ema(ctx, 2, arr, 1, *(hp + (ema, cf(step), scratch, ctypes.c_size_t(nbytes))))
    one = lambda p: (ctypes.c_void_p * 1)(p)
    # each refusal with its own text (the text is per thread and holds until the next failure: it is read right after the call)
    cases = [(lambda: multi(None, 0.1), b'null shadow array'), (lambda: multi(one(sh), -0.1), b'not in [0, 1]'),
             (lambda: multi(one(sh), 1.5), b'not in [0, 1]'), (lambda: multi(one(sh), float('nan')), b'not in [0, 1]'),
             (lambda: multi(one(sh), float('inf')), b'not in [0, 1]'), (lambda: multi(one(sh + 4), 0.1), b'misaligned'),
             (lambda: multi(one(w), 0.1), b'overlaps'), (lambda: multi(one(g + 16), 0.1), b'overlaps'),
             (lambda: multi(one(s0 - 16), 0.1), b'overlaps'), (lambda: multi(one(s1 + 4 * n - 16), 0.1), b'overlaps'),
             (lambda: multi(one(sh), 0.1, nbytes=sb - 1), b'scratch too small')]
    P = ctypes.c_void_p
    cases += [(lambda: L.y3_ema_update(ctx, None, P(w), n, cf(0.1)), b'null argument'),
              (lambda: L.y3_ema_update(ctx, P(sh), P(w), 0, cf(0.1)), b'empty tensor'),
              (lambda: L.y3_ema_update(ctx, P(sh), P(w), n, cf(1.01)), b'not in [0, 1]'),
              (lambda: L.y3_ema_update(ctx, P(sh), P(w), n, cf(float('nan'))), b'not in [0, 1]'),
              (lambda: L.y3_ema_update(ctx, P(w + 4 * n - 4), P(w), n, cf(0.1)), b'overlaps'),
              (lambda: L.y3_ema_update(ctx, P(w), P(w), n, cf(0.1)), b'overlaps')]
    for i, (call, text) in enumerate(cases):
        assert call() == _lib.Y3_EINVAL, i
        assert text in L.y3_last_error(), (i, text, L.y3_last_error())


def test_checkpoint_round_trip_of_the_averages(tmp_path):
    """Saver.save(averages=) stores '<variable>/ExponentialMovingAverage' for the averaged variables and keeps the RAW value
    under the variable's own key, also inside averaged(); restore(averages=) loads the keys that are there and match in
    shape; restore(use_ema=True) puts the average into the variable and falls back to the variable's own key."""
    from yolov3_tensorflow_amd.utils import misc_utils
    src = _variables()
    averaged = {src[0].op_name, src[2].op_name, src[3].op_name}
    tr = _trainer(src, averaged, ema_decay=0.9)
    raw = {v.op_name: v.numpy().copy() for v in src}
    # shadows start as copies of their variables; move them away so that the two are told apart
    assert sorted(tr.ema_tensors()) == sorted(averaged)
    for k, t in tr.ema_tensors().items():
        assert np.array_equal(t.numpy(), raw[k]) and t.data_ptr() != [v for v in src if v.op_name == k][0].tensor.data_ptr()
        t.add_(1.0)
    avg = {k: t.numpy().copy() for k, t in tr.ema_tensors().items()}
    p_out = misc_utils.Saver(src).save(str(tmp_path / 'outside'), global_step=5.0, averages=tr)
    versions = [v.version for v in src]
    with tr.averaged():
        for v in src:       # inside: the averaged variables hold their averages, every one of them was touch()ed
            np.testing.assert_array_equal(v.numpy(), avg.get(v.op_name, raw[v.op_name]))
        assert [v.version > n for v, n in zip(src, versions)] == [v.op_name in averaged for v in src]
        for call in (tr.backward, tr.apply_gradients, lambda: tr.step(None, None)):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(RuntimeError):
            with tr.averaged():
                pass
        p_in = misc_utils.Saver(src).save(str(tmp_path / 'inside'), global_step=5.0, averages=tr)
    for v in src:           # after: the raw values, in the tensors they were in
        np.testing.assert_array_equal(v.numpy(), raw[v.op_name])
    for path in (p_out, p_in):
        ckpt = np.load(path)
        assert sorted(ckpt.files) == sorted(list(raw) + [k + E.EMA_SUFFIX for k in averaged] + ['global_step'])
        for k in raw:
            np.testing.assert_array_equal(ckpt[k], raw[k])
        for k in averaged:
            np.testing.assert_array_equal(ckpt[k + E.EMA_SUFFIX], avg[k])
    assert misc_utils.has_averages(p_in)
    # without the argument the file is what it always was
    plain = misc_utils.Saver(src).save(str(tmp_path / 'plain'), global_step=5.0)
    assert sorted(np.load(plain).files) == sorted(list(raw) + ['global_step']) and not misc_utils.has_averages(plain)

    # restore into a trainer whose shadows exist: present + matching keys are loaded, the others keep their start value
    dst = _variables(seed=1)
    dst[2] = CpuVar(dst[2].op_name, np.zeros((1, 1, 4, 5), np.float32))
    tr2 = _trainer(dst, {dst[0].op_name, dst[1].op_name, dst[2].op_name}, ema_decay=0.9)
    start1 = tr2.ema_tensors()[dst[1].op_name].numpy().copy()
    assert misc_utils.Saver(dst).restore(p_in, averages=tr2) == 5.0
    for v in dst:
        np.testing.assert_array_equal(v.numpy(), raw[v.op_name])
    got = tr2.ema_tensors()
    np.testing.assert_array_equal(got[dst[0].op_name].numpy(), avg[dst[0].op_name])
    np.testing.assert_array_equal(got[dst[2].op_name].numpy(), avg[dst[2].op_name])
    np.testing.assert_array_equal(got[dst[1].op_name].numpy(), start1)            # (the file has no average of the bias)
    assert dst[3].op_name not in got                                              # (this trainer does not update gamma)
    # ... and into one whose shadows do not exist yet (train.py restores before the first step): they start with the stored value
    from yolov3_tensorflow_amd import training
    dst3 = _variables(seed=2)
    tr3 = training.Trainer(None, training.Optimizer('sgd', 1e-3), ema_decay=0.9)
    misc_utils.Saver(dst3).restore(p_in, variables=False, averages=tr3)
    np.testing.assert_array_equal(dst3[0].numpy(), _variables(seed=2)[0].numpy())  # variables=False left the variables alone
    tr3.order = dst3[:2]
    tr3._alloc_ema()
    np.testing.assert_array_equal(tr3.ema_tensors()[dst3[0].op_name].numpy(), avg[dst3[0].op_name])
    np.testing.assert_array_equal(tr3.ema_tensors()[dst3[1].op_name].numpy(), dst3[1].numpy())
    # a trainer without averaging ignores the argument
    tr4 = training.Trainer(None, training.Optimizer('sgd', 1e-3))
    misc_utils.Saver(_variables(seed=3)).restore(p_in, averages=tr4)
    assert tr4.ema_tensors() == {}

    # use_ema: the average where the file has one, the variable's own key elsewhere; on a file without averages, the raw weights
    ev = _variables(seed=4)
    misc_utils.Saver(ev).restore(p_in, use_ema=True)
    for v in ev:
        np.testing.assert_array_equal(v.numpy(), avg.get(v.op_name, raw[v.op_name]))
    ev = _variables(seed=4)
    misc_utils.Saver(ev).restore(plain, use_ema=True)
    for v in ev:
        np.testing.assert_array_equal(v.numpy(), raw[v.op_name])


def test_restore_for_inference_says_when_there_are_no_averages(tmp_path, capsys):
    from yolov3_tensorflow_amd.utils import misc_utils
    src = _variables()
    tr = _trainer(src, {src[0].op_name}, ema_decay=0.9)
    tr.ema_tensors()[src[0].op_name].mul_(2.0)
    with_avg = misc_utils.Saver(src).save(str(tmp_path / 'with'), averages=tr)
    without = misc_utils.Saver(src).save(str(tmp_path / 'without'))
    ev = _variables(seed=5)
    misc_utils.restore_for_inference(ev, with_avg, use_ema=True)
    assert 'no weight moving averages' not in capsys.readouterr().out
    np.testing.assert_array_equal(ev[0].numpy(), 2.0 * src[0].numpy())
    np.testing.assert_array_equal(ev[1].numpy(), src[1].numpy())
    misc_utils.restore_for_inference(ev, without, use_ema=True)
    assert 'holds no weight moving averages' in capsys.readouterr().out
    np.testing.assert_array_equal(ev[0].numpy(), src[0].numpy())
    misc_utils.restore_for_inference(ev, with_avg)
    assert capsys.readouterr().out == ''
    np.testing.assert_array_equal(ev[0].numpy(), src[0].numpy())


def test_strip_tool_drops_the_averages_or_moves_them_into_the_variables(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'misc'))
    import remove_optimizers_params_in_ckpt as rm
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils import misc_utils
    src = _variables()
    averaged = {src[0].op_name, src[3].op_name}
    tr = _trainer(src, averaged, ema_decay=0.9)
    for t in tr.ema_tensors().values():
        t.sub_(3.0)
    opt = training.Optimizer('momentum', 1e-3)
    opt.slots[src[0].op_name] = (torch.ones(src[0].shape), None)
    path = misc_utils.Saver(src).save(str(tmp_path / 'full'), optimizer=opt, global_step=9.0, averages=tr)
    names = sorted(v.op_name for v in src)
    for use_ema, out in ((False, 'raw.npz'), (True, 'ema.npz')):
        keep, drop = rm.main([path, '--output', str(tmp_path / out)] + (['--use_ema', 'true'] if use_ema else []))
        assert sorted(keep) == names
        assert sorted(drop) == sorted([k + E.EMA_SUFFIX for k in averaged] + [src[0].op_name + '/Momentum', 'global_step',
                                                                            'optimizer/step'])
        got = np.load(str(tmp_path / out))
        assert sorted(got.files) == names
        for v in src:
            want = v.numpy() - 3.0 if use_ema and v.op_name in averaged else v.numpy()
            np.testing.assert_array_equal(got[v.op_name], want)
    # the --use_ema file is a plain checkpoint: the demo scripts' own restore (no option of theirs) loads the averages from it
    sys.path.insert(0, ROOT)
    import test_single_image
    ev = _variables(seed=6)
    assert test_single_image.restore(ev, str(tmp_path / 'ema.npz'))
    for v, s in zip(ev, src):
        np.testing.assert_array_equal(v.numpy(), s.numpy() - 3.0 if s.op_name in averaged else s.numpy())


def test_scripts_take_the_options():
    sys.path.insert(0, ROOT)
    import eval as eval_script
    import train as train_script
    a = train_script.build_parser().parse_args([])
    assert a.ema_decay == 0 and a.ema_warmup is True
    a = train_script.build_parser().parse_args(['--ema_decay', '0.9998', '--ema_warmup', 'false'])
    assert a.ema_decay == 0.9998 and a.ema_warmup is False
    assert eval_script.build_parser().parse_args([]).use_ema is False
    assert eval_script.build_parser().parse_args(['--use_ema', 'true']).use_ema is True
