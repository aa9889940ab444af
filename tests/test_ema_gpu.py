"""The weight moving average on the device (include/yolo355.h, "Weight moving average"): y3_clip_update_multi_ema against
y3_clip_update_multi (w, g and the slots: the same bits) and against the fp64 rule (the shadows), y3_ema_update, the guarded
arena, training.Trainer(ema_decay=...) with averaged(), and train.py / eval.py end to end.

The shadow gate is derived, not tuned (ema_cases.bound): at most three fp32 roundings with |ema_step| <= 1 give
5 * 2^-24 * max(|shadow|, |w_new|) per element and update.  The rule's input is the GPU's own new w, which assertion 1 ties bit
for bit to the kernel that test_optimizer_gpu holds to the oracle.  Measured on the MI355X (the tests print it): the worst
element is 0.43-0.45 bounds away in the kernel tests under every rule, 0.20 of the three-step gate in the Trainer test; the
perturbed references are 5.4e6-6.7e6 bounds away (1 - ema_step) and 1.6e5-1.1e7 (old w) under ema_step 0.1 and 0.9; under 2e-4
the old-w reference is 1416 (sgd), 2473 (momentum), 718 (adam) and 322 (rmsprop) bounds away; the per-tensor path gave the
fused path's w for 66 of 66 variables.

Sensitivity guards run NO broken kernel: references with ema_step replaced by 1 - ema_step, and with the old w in place of the
new one, are built on the CPU and must lie more than 100 bounds from what the GPU produced."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import COCO_ANCHORS, ROOT, blob_images
import ema_cases as E
import test_optimizer_gpu as TO

pytestmark = pytest.mark.gpu


# ---- the kernels -------------------------------------------------------------------------------------------------------------
def _upload(kind, dev):
    """device copies of ema_cases.inputs(kind): tensors of their own, and ONE flat buffer that holds every shadow at exactly
    its contract alignment (a NULL-shadow tensor's place is filled with SENTINEL)"""
    ins = E.inputs(kind)
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)
    ts = [dict(w=up(t['w']), g=up(t['g']), s0=up(t['s0']), s1=up(t['s1']), wd=t['wd']) for t in ins]
    offs, total = E.shadow_layout()
    flat = np.full(total, E.SENTINEL, np.float32)
    for t, o in zip(ins, offs):
        if t['shadow'] is not None:
            flat[o:o + t['shadow'].size] = t['shadow']
    flat_dev = torch.from_numpy(flat.copy()).to(dev)
    assert flat_dev.data_ptr() % 64 == 0
    for t, n, o in zip(ts, E.SIZES, offs):
        t['shadow'] = flat_dev[o:o + n]
        assert t['shadow'].data_ptr() % (32 if n % 4 == 0 else 8) == (16 if n % 4 == 0 else 4)
    return ins, ts, flat, flat_dev


def _multi(kind, ts, ema_step=None, null=E.NO_SHADOW):
    """y3_clip_update_multi (ema_step None) or y3_clip_update_multi_ema on the device tensors, in place"""
    from yolov3_tensorflow_amd import framework as fw, _lib
    L, ctx = _lib.lib(), fw.context()
    arr = (_lib.ParamDesc * len(ts))()
    dp = lambda a: 0 if a is None else a.data_ptr()
    for i, t in enumerate(ts):
        arr[i] = _lib.ParamDesc(dp(t['w']), dp(t['g']), dp(t['s0']), dp(t['s1']), t['w'].numel(), t['wd'], 0)
    k = TO.KINDS.index(kind)
    if ema_step is None:
        sc = torch.empty(L.y3_clip_update_multi_scratch_bytes(arr, len(ts)), dtype=torch.uint8, device=ts[0]['w'].device)
        _lib.check(L.y3_clip_update_multi(ctx, k, arr, len(ts), *(E.hyper(kind) + (fw.ptr(sc), ctypes.c_size_t(sc.numel())))))
    else:
        ema = (ctypes.c_void_p * len(ts))(*[None if i in null else t['shadow'].data_ptr() for i, t in enumerate(ts)])
        sc = torch.empty(L.y3_clip_update_multi_ema_scratch_bytes(arr, len(ts)), dtype=torch.uint8, device=ts[0]['w'].device)
        _lib.check(L.y3_clip_update_multi_ema(ctx, k, arr, len(ts), *(E.hyper(kind) + (ema, ctypes.c_float(ema_step), fw.ptr(sc),
                                                                                   ctypes.c_size_t(sc.numel())))))
    torch.cuda.synchronize()


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('kind', TO.KINDS)
def test_fused_update_keeps_the_plain_outputs_and_moves_the_shadows_by_the_rule(kind):
    """All of ema_cases.SIZES in one call, from warm slots, for each of the three step factors.
    1. w, g, slot0, slot1: bit-identical to y3_clip_update_multi on copies of the same inputs.
    2. every shadow within ema_cases.bound of the fp64 rule on (its start value, the GPU's new w).
    3. ema_step = 0 keeps every shadow's bits; the places of the NULL-shadow tensors (between real shadows in one buffer) keep
       theirs under every step; y3_ema_update on (shadow start, new w) gives the fused kernel's bits.
    Guards: 1 - ema_step for ema_step, and the old w for the new one, each more than 100 bounds away under every step."""
    from yolov3_tensorflow_amd import framework as fw, _lib
    dev = fw.default_device()
    ins, plain, _, _ = _upload(kind, dev)
    _multi(kind, plain)
    want = [{k: None if t[k] is None else t[k].cpu().numpy() for k in ('w', 'g', 's0', 's1')} for t in plain]
    offs, total = E.shadow_layout()
    worst, guards = 0.0, {}
    for step in E.EMA_STEPS + (0.0,):
        _, ts, flat0, flat_dev = _upload(kind, dev)
        _multi(kind, ts, step)
        flat1 = flat_dev.cpu().numpy()
        for i, (t, e) in enumerate(zip(ts, want)):                                   # 1
            for key in ('w', 'g', 's0', 's1'):
                assert (t[key] is None) == (e[key] is None)
                if e[key] is not None:
                    assert _bits(t[key].cpu().numpy(), e[key]), '%s of tensor %d (n = %d), ema_step %g' % (key, i, E.SIZES[i], step)
        covered = np.zeros(total, bool)
        for i, (t, o, n) in enumerate(zip(ins, offs, E.SIZES)):
            if t['shadow'] is None:
                continue
            covered[o:o + n] = True
            got, w_new = flat1[o:o + n], want[i]['w']
            if step == 0.0:                                                          # 3
                assert _bits(got, t['shadow']), i
                continue
            bnd = E.bound(t['shadow'], w_new)
            r = E.worst_ratio(got, E.ema64(t['shadow'], w_new, step), bnd)           # 2
            worst = max(worst, r)
            assert r <= 1.0, 'shadow of tensor %d (n = %d), ema_step %g: %.2f bounds' % (i, n, step, r)
        assert _bits(flat1[~covered], flat0[~covered]), 'a byte outside the shadows changed (ema_step %g)' % step      # 3
        if step == 0.0:
            continue
        # the stand-alone entry on the same (shadow, w_new): the same bits
        L, ctx = _lib.lib(), fw.context()
        for i, (t, o, n) in enumerate(zip(ins, offs, E.SIZES)):
            if t['shadow'] is None:
                continue
            s = torch.from_numpy(t['shadow'].copy()).to(dev)
            _lib.check(L.y3_ema_update(ctx, fw.ptr(s), fw.ptr(ts[i]['w']), n, ctypes.c_float(step)))
            torch.cuda.synchronize()
            assert _bits(s.cpu().numpy(), flat1[o:o + n]), 'y3_ema_update differs from the fused kernel on tensor %d' % i
        # guards (no broken kernel runs)
        far = dict(one_minus_step=0.0, old_w=0.0)
        for i, (t, o, n) in enumerate(zip(ins, offs, E.SIZES)):
            if t['shadow'] is None:
                continue
            bnd = E.bound(t['shadow'], want[i]['w'])
            far['one_minus_step'] = max(far['one_minus_step'], E.worst_ratio(flat1[o:o + n], E.ema64(t['shadow'], want[i]['w'], 1.0 - E.f32(step)), bnd))
            far['old_w'] = max(far['old_w'], E.worst_ratio(flat1[o:o + n], E.ema64(t['shadow'], t['w'], step), bnd))
        guards[step] = far
        assert far['one_minus_step'] > E.GUARD, 'ema_step %g: 1 - ema_step would pass: %s' % (step, far)
        # (the old-w reference is ema_step * |w_new - w_old| from the rule: ema_cases.inputs gives every rule, Adam included, an
        # element that moves far enough for the smallest step)
        assert far['old_w'] > E.GUARD, 'ema_step %g: the old w would pass: %s' % (step, far)
    print('ema %s: worst shadow error %.3f bounds; guards (bounds away) %s' % (kind, worst, ', '.join(
        '%g: %.0f / %.0f' % (s, g['one_minus_step'], g['old_w']) for s, g in guards.items())))


@pytest.mark.parametrize('kind', TO.KINDS)
def test_fused_update_in_a_guarded_arena(kind):
    """The mixed-size call between poisoned guards (tests/guarded.py, as test_guard_bands_gpu.py runs the plain update):
    shadows `inout` at exactly their contract alignment, the scratch with exactly the bytes of the new query, two poison
    passes; no guard byte changes, both passes give the same bits, and the results hold their gates."""
    import guarded
    import test_guard_bands_gpu as TG
    g = TG.G()
    run = E.guard_band_multi(g, kind, ema_step=E.EMA_STEPS[1])
    assert any(s.name.startswith('shadow') and s.align == 4 for s in run.specs) and any(
        s.name.startswith('shadow') and s.align == 16 for s in run.specs)
    arena = guarded.build(g.dev, run.specs)
    kept = guarded.run_passes(arena, lambda: run.call(arena), run.outputs, sync=torch.cuda.synchronize)
    g.fw.check_context()
    assert g.called == {'y3_clip_update_multi_ema'}
    guarded.assert_passes_identical(kept, 'clip_update_multi_ema-%s' % kind)
    run.verify(kept[0])


# ---- training.Trainer ------------------------------------------------------------------------------------------------------
N, HW, CLASSES, STEPS, DECAY = 2, 64, 80, 3, 0.9
HEAD = 'yolov3/yolov3_head'


def _model_and_data():
    import yolov3_tensorflow_amd as y3
    from oracle import yolo_ref, train_ref
    params = yolo_ref.synthetic_params(CLASSES, seed=1)
    y3.reset_default_graph()
    model = y3.yolov3(CLASSES, COCO_ANCHORS, batch_norm_decay=0.99, weight_decay=5e-4)
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    for v in y3.global_variables(scope='yolov3'):
        v.assign(params[v.op_name])
    dev = y3.global_variables(scope='yolov3')[0].tensor.device
    x = torch.from_numpy(blob_images(11, N, HW)).to(dev)
    yts = [torch.from_numpy(np.ascontiguousarray(y)).to(dev)
           for y in train_ref.synthetic_targets(12, N, [HW, HW], CLASSES, COCO_ANCHORS, max_boxes=3)]
    return model, params, x, yts


def _run_steps(ema_decay, steps=STEPS, inside=None, per_tensor=False, monkeypatch=None):
    """`steps` Trainer.step calls (momentum, head scope, batch 2 at 64 px) from the synthetic weights.  Returns the trainer,
    the losses, the head variables after every step, and the final variables / slots.  inside(trainer, model, x): called
    after the last step (for the averaged() checks), before one FURTHER step whose result is returned too."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    model, params, x, yts = _model_and_data()
    upd = [v for v in y3.global_variables(scope='yolov3') if v.op_name.startswith(HEAD + '/') and v.trainable]
    trainer = training.Trainer(model, training.Optimizer('momentum', 1e-3, momentum=0.9), update_vars=upd, wgrad_stream=False,
                               ema_decay=ema_decay)
    if per_tensor:
        monkeypatch.setenv('Y3_TRAIN_PER_TENSOR_UPDATE', '1')
    losses, ws = [], []
    start = {v.op_name: v.numpy().copy() for v in upd}
    with y3.variable_scope('yolov3'):
        for _ in range(steps):
            losses.append(torch.stack(trainer.step(x, yts)).cpu().numpy())
            ws.append({v.op_name: v.numpy().copy() for v in upd})
        extra = None
        if inside is not None:
            inside(trainer, model, x, yts)
            extra = torch.stack(trainer.step(x, yts)).cpu().numpy()
    torch.cuda.synchronize()
    final = {v.op_name: v.numpy().copy() for v in y3.global_variables(scope='yolov3')}
    slots = {k: s[0].cpu().numpy().copy() for k, s in trainer.opt.slots.items()}
    return dict(trainer=trainer, losses=losses, ws=ws, start=start, final=final, slots=slots, extra=extra, params=params,
                names=[v.op_name for v in upd])


def _chain(run):
    """the fp64 rule chained on the CPU over the observed w values, at the floats the ABI carried; and the gate: the
    per-step bound summed over the steps (each on that step's shadow and w)"""
    tr = run['trainer']
    shadow = {k: v.astype(np.float64) for k, v in run['start'].items()}
    gate = {k: np.zeros_like(v) for k, v in shadow.items()}
    for t, ws in enumerate(run['ws']):
        for k in shadow:
            gate[k] += E.bound(shadow[k], ws[k])
            shadow[k] = E.ema64(shadow[k], ws[k], tr.ema_step_at(t))
    return shadow, gate


def test_trainer_keeps_the_averages_and_leaves_the_step_alone(isolated_graph):
    """Three Trainer.step calls at the smallest legal input (batch 2 at 64 px), update_vars = the head scope, with
    ema_decay = 0.9 and without: variables, slots and losses bit-identical; the shadows equal the fp64 rule chained over the
    three observed w values within three per-step bounds; inside averaged() the inference forward is that of a model that was
    ASSIGNED the shadow values, step() raises, and afterwards the variables' bits and a further step are those of the run that
    never entered the context."""
    import yolov3_tensorflow_amd as y3
    seen = {}

    def inside(trainer, model, x, yts):
        before = {v.op_name: (v.tensor.data_ptr(), v.numpy().copy()) for v in trainer.order}
        avg = {k: t.cpu().numpy().copy() for k, t in trainer.ema_tensors().items()}
        seen['raw'] = {v.op_name: v.numpy().copy() for v in y3.global_variables(scope='yolov3')}
        with trainer.averaged():
            for v in trainer.order:
                assert _bits(v.numpy(), avg[v.op_name])
            seen['others'] = {v.op_name: v.numpy().copy() for v in y3.global_variables(scope='yolov3')}
            seen['fms'] = [f.cpu().numpy().copy() for f in model.forward(x, is_training=False)]
            with pytest.raises(RuntimeError):
                trainer.step(x, yts)
            with pytest.raises(RuntimeError):
                trainer.apply_gradients()
        for v in trainer.order:
            assert v.tensor.data_ptr() == before[v.op_name][0] and _bits(v.numpy(), before[v.op_name][1])
        seen['avg'] = avg

    on = _run_steps(DECAY, inside=inside)
    off = _run_steps(None, inside=lambda *a: None)
    assert len(on['names']) > 20 and off['trainer'].ema is None
    for a, b in zip(on['losses'] + [on['extra']], off['losses'] + [off['extra']]):
        assert np.isfinite(a).all() and _bits(a, b)
    for k in off['final']:
        assert _bits(on['final'][k], off['final'][k]), k
    assert sorted(on['slots']) == sorted(off['slots'])
    for k in off['slots']:
        assert _bits(on['slots'][k], off['slots'][k]), k
    assert on['trainer'].global_step == off['trainer'].global_step == STEPS + 1
    # the shadows after three steps
    tr = on['trainer']
    assert [tr.ema_step_at(t) for t in range(3)] == [1 - 0.1, 1 - 2.0 / 11.0, 1 - 3.0 / 12.0]      # the ramp: d_t < 0.9 here
    want, gate = _chain(on)
    assert sorted(seen['avg']) == sorted(on['names'])
    worst, far = 0.0, 0.0
    for k in on['names']:
        r = E.worst_ratio(seen['avg'][k], want[k], gate[k])
        worst = max(worst, r)
        assert r <= 1.0, '%s: %.2f of the three-step gate' % (k, r)
        # guard: the rule fed the w BEFORE each step instead of the new one
        old = on['start'][k].astype(np.float64)
        for t in range(STEPS):
            old = E.ema64(old, on['start'][k] if t == 0 else on['ws'][t - 1][k], tr.ema_step_at(t))
        far = max(far, E.worst_ratio(seen['avg'][k], old, gate[k]))
    assert far > E.GUARD, far
    print('trainer shadows: worst %.3f of the three-step gate; old-w chain %.0f gates away' % (worst, far))
    # a second model that was assigned the shadow values gives the same inference forward
    model2, _, x, _ = _model_and_data()
    for v in y3.global_variables(scope='yolov3'):
        v.assign(seen['avg'].get(v.op_name, seen['others'][v.op_name]))
    with y3.variable_scope('yolov3'):
        fms2 = [f.cpu().numpy() for f in model2.forward(x, is_training=False)]
    for a, b in zip(seen['fms'], fms2):
        assert np.isfinite(a).all() and _bits(a, b)
    # ... and not the forward of the raw weights
    for v in y3.global_variables(scope='yolov3'):
        v.assign(seen['raw'][v.op_name])
    with y3.variable_scope('yolov3'):
        raw_fms = [f.cpu().numpy() for f in model2.forward(x, is_training=False)]
    assert not any(_bits(a, b) for a, b in zip(seen['fms'], raw_fms))


def test_per_tensor_update_path_gives_the_fused_shadows(isolated_graph, monkeypatch):
    """Y3_TRAIN_PER_TENSOR_UPDATE=1 (y3_clip_update, then y3_ema_update, per variable) after three steps: the shadows of the
    fused path, bit for bit, for every variable.  That needs the two update paths to give the same w at every step, which is
    asserted first: y3_clip_update sums the squared gradient in another order than the multi-tensor call, so a clipped
    tensor's w could differ in the last bit, and an average of other inputs is another average; on this seed none does (66
    of 66 variables).  Every shadow of the per-tensor path is also within the three-step gate of the fp64 rule chained over
    its observed w."""
    fused = _run_steps(DECAY)
    avg_fused = {k: t.cpu().numpy().copy() for k, t in fused['trainer'].ema_tensors().items()}
    single = _run_steps(DECAY, per_tensor=True, monkeypatch=monkeypatch)
    avg_single = {k: t.cpu().numpy().copy() for k, t in single['trainer'].ema_tensors().items()}
    assert sorted(avg_fused) == sorted(avg_single) == sorted(fused['names'])
    want, gate = _chain(single)
    same_w = [k for k in fused['names'] if all(_bits(a[k], b[k]) for a, b in zip(fused['ws'], single['ws']))]
    print('per-tensor path: %d of %d variables with the fused path\'s w at every step' % (len(same_w), len(fused['names'])))
    assert len(same_w) == len(fused['names'])      # (observed for this seed: no head tensor's clipped w differs between the paths)
    for k in fused['names']:
        assert E.worst_ratio(avg_single[k], want[k], gate[k]) <= 1.0, k
        assert _bits(avg_fused[k], avg_single[k]), k
    assert any(not _bits(avg_fused[k], fused['final'][k]) for k in fused['names'])      # (averages, not the last iterate)


# ---- train.py / eval.py ----------------------------------------------------------------------------------------------------
def test_train_script_saves_resumes_and_evaluates_the_averages(tmp_path, capsys, isolated_graph, monkeypatch):
    """Two epochs of train.main on the 8-image set of test_train_script_gpu with --ema_decay 0.9: the best-model .npz holds the
    averages beside the raw weights; a second train.main resuming from it starts with those shadows; eval.py --use_ema true
    on the file runs, reports, and evaluates other weights than without the flag."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from test_train_script_gpu import make_dataset
    sys.path.insert(0, ROOT)
    import train as train_script
    import eval as eval_script
    ann, names = make_dataset(tmp_path)
    anchors = os.path.join(ROOT, 'data', 'yolo_anchors.txt')
    common = ['--train_file', ann, '--val_file', ann, '--anchor_path', anchors, '--class_name_path', names, '--batch_size', '4',
              '--img_size', '64', '64', '--letterbox_resize', 'false', '--train_evaluation_step', '1000',
              '--batch_norm_decay', '0.9', '--save_epoch', '1000', '--optimizer_name', 'momentum', '--learning_rate_init', '1e-3',
              '--lr_type', 'fixed', '--update_part', 'yolov3/yolov3_head', '--multi_scale_train', 'false', '--use_warm_up', 'false',
              '--warm_up_epoch', '0', '--use_label_smooth', 'false', '--use_focal_loss', 'false', '--weight_decay', '0',
              '--augment', 'false', '--num_threads', '2', '--progress_log_path', '', '--ema_decay', '0.9']
    started = []
    alloc = training.Trainer._alloc_ema

    def recording(self):
        fresh = self.ema is None
        alloc(self)
        if fresh and self.ema is not None:
            started.append({k: t.cpu().numpy().copy() for k, t in self.ema.items()})
    monkeypatch.setattr(training.Trainer, '_alloc_ema', recording)

    y3.reset_default_graph()
    hist = train_script.main(common + ['--restore_path', '', '--save_dir', str(tmp_path / 'ckpt'), '--total_epoches', '2',
                                       '--val_evaluation_epoch', '1'])
    assert np.isfinite(hist['loss']).all() and len(hist['loss']) == 4 and len(hist['mAP']) == 2
    files = sorted(os.listdir(str(tmp_path / 'ckpt')))
    npz = [f for f in files if f.startswith('best_model_') and f.endswith('.npz')]
    assert npz and any(f.endswith('.weights') for f in files)
    path = str(tmp_path / 'ckpt' / npz[-1])
    ckpt = np.load(path)
    avg_keys = [k for k in ckpt.files if k.endswith(E.EMA_SUFFIX)]
    head = [v.op_name for v in y3.global_variables(scope='yolov3') if v.op_name.startswith('yolov3/yolov3_head/') and v.trainable]
    assert sorted(avg_keys) == sorted(k + E.EMA_SUFFIX for k in head)
    moved = [k for k in head if not np.array_equal(ckpt[k], ckpt[k + E.EMA_SUFFIX])]
    assert moved                              # (the raw weights under their own names, the averages beside them)
    # the first run's shadows started as copies of the initial variables; the resumed run's start with the stored averages
    y3.reset_default_graph()
    hist2 = train_script.main(common + ['--restore_path', path, '--restore_exclude', 'None', '--save_dir', str(tmp_path / 'ckpt2'),
                                        '--total_epoches', '1', '--val_evaluation_epoch', '1000'])
    assert hist2['global_step_start'] == int(ckpt['global_step']) and len(started) == 2
    assert sorted(started[1]) == sorted(head)
    for k in head:
        assert _bits(started[1][k], ckpt[k + E.EMA_SUFFIX]), k
    capsys.readouterr()
    # eval.py on the file, with and without the averages
    ev = ['--eval_file', ann, '--restore_path', path, '--anchor_path', anchors, '--class_name_path', names, '--img_size', '64', '64',
          '--batch_size', '8', '--num_threads', '2', '--compute_dtype', 'f32']
    y3.reset_default_graph()
    out_ema = eval_script.main(ev + ['--use_ema', 'true'])
    text = capsys.readouterr().out
    assert 'final mAP' in text and 'no weight moving averages' not in text
    y3.reset_default_graph()
    out_raw = eval_script.main(ev)
    assert np.isfinite(out_ema['loss']).all() and np.isfinite(out_raw['loss']).all() and out_ema['loss'][0] != out_raw['loss'][0]
    # a file without averages: said so, and evaluated as it is
    sys.path.insert(0, os.path.join(ROOT, 'misc'))
    import remove_optimizers_params_in_ckpt as rm
    rm.main([path, '--output', str(tmp_path / 'stripped.npz')])
    capsys.readouterr()
    y3.reset_default_graph()
    out_stripped = eval_script.main(ev[:2] + ['--restore_path', str(tmp_path / 'stripped.npz')] + ev[4:] + ['--use_ema', 'true'])
    assert 'holds no weight moving averages' in capsys.readouterr().out
    assert out_stripped['loss'] == out_raw['loss']
