"""GPU tests of the device VOC evaluator: y3_voc_append / y3_voc_match / y3_voc_ap (include/yolo355.h) and
eval_utils.DeviceEval against eval_utils.voc_eval, held to the equalities of tests/test_voc_device_cpu.py (npos, nd, recall,
precision and the 11-point AP bit for bit; the area AP within nd * 2**-52), plus what only the kernels have: the append's
order and capacity, segments longer than one pass of the AP kernel, an image with more objects than a wavefront is wide, and
run-to-run identity."""
import ctypes
import os
import sys

import numpy as np
import pytest

import voc_cases as vc
from device_eval_helpers import eval_script_set, nms_like

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _c_entries(case, iou_thres, use_07_metric, pad_rows=5):
    """The table through y3_voc_match + y3_voc_ap with the arena loaded directly (float64 rows), `pad_rows` dead rows behind the
    detections (the device count word says how many are live).  Returns (table, tp in rank order, order)."""
    import torch
    from yolov3_tensorflow_amd import _lib, framework as fw
    L, dev = _lib.lib(), fw.default_device()
    a = vc.arena_of(case)
    n, R, C = len(case.preds), len(case.preds) + pad_rows, case.class_num
    pad = lambda x, fill: torch.from_numpy(np.concatenate([x, np.full((pad_rows,) + x.shape[1:], fill, x.dtype)])).to(dev)
    box, score, label, image = pad(a['box'], 1e9), pad(a['score'], 2.0), pad(a['label'], 0), pad(a['image'], 10 ** 6)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    live = torch.arange(R, device=dev) < n
    by_score = torch.sort(-score, stable=True).indices
    key = torch.where(live, label, torch.full_like(label, C))[by_score]
    order = by_score[torch.sort(key, stable=True).indices].to(torch.int32).contiguous()
    gt_start, gt_box, gt_label = (torch.from_numpy(a[k]).to(dev) for k in ('gt_start', 'gt_box', 'gt_label'))
    mb, ab = L.y3_voc_match_scratch_bytes(R, a['num_gt']), L.y3_voc_ap_scratch_bytes(R)
    scratch = torch.empty(max(mb, ab), dtype=torch.uint8, device=dev)
    tp = torch.full((R,), 9, dtype=torch.uint8, device=dev)
    seg = torch.full((C + 1,), -1, dtype=torch.int32, device=dev)
    out = torch.full((C, 5), -7., dtype=torch.float64, device=dev)
    ctx = fw.context(dev)
    _lib.check(L.y3_voc_match(ctx, fw.ptr(box), fw.ptr(label), fw.ptr(image), fw.ptr(order), R, fw.ptr(count), fw.ptr(gt_start),
                              fw.ptr(gt_box), fw.ptr(gt_label), a['num_images'], a['num_gt'], C, iou_thres, fw.ptr(scratch), mb,
                              fw.ptr(tp), fw.ptr(seg)))
    thr = (ctypes.c_double * 11)(*np.arange(0., 1.1, 0.1))
    _lib.check(L.y3_voc_ap(ctx, fw.ptr(tp), fw.ptr(seg), R, fw.ptr(gt_label), a['num_gt'], C, int(use_07_metric), thr,
                           fw.ptr(scratch), ab, fw.ptr(out)))
    tp = tp.cpu().numpy()
    assert (tp[n:] == 0).all()
    return out.cpu().numpy(), tp[:n], order.cpu().numpy()[:n]


def _device_eval(case, batches=None, cap=64, **kw):
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    ev = DeviceEval(case.gt_dict, case.image_ids, case.class_num, **kw)
    rows = []
    for ids in batches or [case.image_ids[i:i + 16] for i in range(0, len(case.image_ids), 16)]:
        dets, r = nms_like(case.preds, ids, cap, fw.default_device())
        ev.add(ids, dets)
        rows += r
    return ev, rows


def test_reference_vectors_through_the_entries_and_device_eval():
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    case, results = vc.golden()
    ev = DeviceEval(case.gt_dict, case.image_ids, case.class_num, capacity_rows=100)
    p = case.preds
    ev.add_rows([r[0] for r in p[:30]], [r[1:5] for r in p[:30]], [r[5] for r in p[:30]], [r[6] for r in p[:30]])
    ev.add_rows([r[0] for r in p[30:]], [r[1:5] for r in p[30:]], [r[5] for r in p[30:]], [r[6] for r in p[30:]])
    for m07 in (False, True):
        want = np.array([r[2:] for r in results if bool(r[1]) == m07], np.float64)
        got, _, _ = _c_entries(case, 0.5, m07)
        vc.assert_table(got, want, m07, 'golden entries m07=%d' % m07)
        assert got[5].tolist() == [1e-6, 1e-6, 0., 0., 0.]
        vc.assert_table(ev.finish(0.5, m07), want, m07, 'golden DeviceEval m07=%d' % m07)


@pytest.mark.parametrize('seed', [1, 2])
def test_random_sets(seed):
    exact = vc.random_case(seed, fp32=False)          # float64 rows straight into the arena
    case = vc.random_case(seed, fp32=True)            # fp32 detections through y3_voc_append
    vc.assert_distinct_scores(case)
    ev, rows = _device_eval(case)
    assert rows == case.preds
    for thres, m07 in ((0.5, False), (0.5, True), (0.3, False)):
        vc.assert_table(_c_entries(exact, thres, m07)[0], vc.reference_table(exact, thres, m07), m07, 'entries %d' % seed)
        vc.assert_table(ev.finish(thres, m07), vc.reference_table(case, thres, m07), m07, 'DeviceEval %d' % seed)


@pytest.mark.parametrize('name', sorted(vc.corner_cases()) + ['tied'])
def test_corner_cases_on_the_device(name):
    if name == 'tied':
        case, expect, fn = vc.tied_case(), None, vc.voc_eval_stable
    else:
        (case, expect), fn = vc.corner_cases()[name], None
    for m07 in (False, True):
        got, tp, order = _c_entries(case, 0.5, m07)
        vc.assert_table(got, vc.reference_table(case, 0.5, m07, fn=fn), m07, name)
        ev, _ = _device_eval(case, cap=len(case.preds))
        vc.assert_table(ev.finish(0.5, m07), vc.reference_table(case, 0.5, m07, fn=fn), m07, name + ' DeviceEval')
    if expect:
        ranked_labels = np.array([case.preds[k][6] for k in order])
        assert tp[ranked_labels == expect[0]].tolist() == expect[1]
    else:
        key = [(case.preds[k][6], -case.preds[k][5], k) for k in order]
        assert key == sorted(key)


def test_append_order_gaps_and_unknown_ids():
    """Three batches with non-contiguous image indices, images without detections in the middle, a per-image capacity far above
    the counts: the arena holds the host concatenation, in order."""
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    case = vc.random_case(4, images=14, classes=4)
    ids = case.image_ids
    quiet = {ids[3], ids[8], ids[9]}
    case = vc.Case(case.gt_dict, ids, [p for p in case.preds if p[0] not in quiet], 4)
    batches = [[ids[11], ids[3], ids[0], ids[7], ids[13]], [ids[9], ids[8], ids[2], ids[12]], [ids[5], ids[1], ids[4], ids[10], ids[6]]]
    ev, rows = _device_eval(case, batches, cap=300, capacity_rows=len(case.preds) + 40)
    box, score, label, image = (t.cpu().numpy() for t in ev._arena)
    state = ev._state.cpu().numpy().tolist()
    n = len(rows)
    assert state == [n, 0] and n == len(case.preds) > 100
    index = {k: i for i, k in enumerate(ids)}
    np.testing.assert_array_equal(box[:n], np.array([r[1:5] for r in rows], np.float64))
    np.testing.assert_array_equal(score[:n], np.array([r[5] for r in rows], np.float64))
    np.testing.assert_array_equal(label[:n], np.array([r[6] for r in rows], np.int32))
    np.testing.assert_array_equal(image[:n], np.array([index[r[0]] for r in rows], np.int32))
    assert (score[n:] == 0).all() and (label[n:] == 0).all()
    by_arrival = vc.Case(case.gt_dict, ids, rows, 4)
    vc.assert_table(ev.finish(), vc.reference_table(by_arrival, 0.5, False), False, 'append')
    with pytest.raises(ValueError):
        ev.add([ids[0], 'nowhere'], nms_like(case.preds, ids[:2], 300, ev._dev)[0])
    with pytest.raises(ValueError):
        DeviceEval(case.gt_dict, ids + [12345], 4)


def test_seventy_objects_of_one_class_in_one_image():
    rng = np.random.RandomState(8)
    objs, preds = [], []
    for k in range(70):
        x0, y0 = 40. * (k % 10), 40. * (k // 10)
        objs.append([x0, y0, x0 + 30., y0 + 30., 0])
    for k in rng.permutation(70)[:60]:      # a jittered detection for most objects, a duplicate for some, clutter
        o = objs[k]
        preds.append([7, o[0] + 1., o[1] - 1., o[2] + 2., o[3], 0., 0])
        if k % 3 == 0:
            preds.append([7, o[0] - 2., o[1] + 2., o[2], o[3] + 1., 0., 0])
    for _ in range(20):
        x0, y0 = rng.uniform(0, 400, 2)
        preds.append([7, x0, y0, x0 + 30., y0 + 30., 0., 0])
    for p, s in zip(preds, rng.permutation(np.linspace(0.05, 0.95, len(preds)))):
        p[5] = float(np.float32(s))
    case = vc.Case({7: objs, 9: []}, [7, 9], [[p[0]] + [float(np.float32(v)) for v in p[1:5]] + p[5:] for p in preds], 1)
    vc.assert_distinct_scores(case)
    for m07 in (False, True):
        want = vc.reference_table(case, 0.5, m07)
        assert want[0, 0] == 70 and 0.5 < want[0, 2] < 1.0
        vc.assert_table(_c_entries(case, 0.5, m07)[0], want, m07, '70 objects')
        vc.assert_table(_device_eval(case, cap=len(preds))[0].finish(0.5, m07), want, m07, '70 objects DeviceEval')


@pytest.fixture(scope='module')
def long_case():
    """Class 0's segment is three passes of the AP kernel plus one rank; class 1 rides behind it."""
    from yolov3_tensorflow_amd import _lib
    pass_len = _lib.lib().y3_voc_ap_pass()
    rng = np.random.RandomState(21)
    gd, preds, want0 = {}, [], 3 * pass_len + 1
    for img in range(64):
        objs = []
        for _ in range(10):
            x0, y0 = rng.uniform(0, 380, 2)
            objs.append([x0, y0, x0 + rng.uniform(10, 90), y0 + rng.uniform(10, 90), int(rng.randint(0, 2))])
        gd[img] = objs
    n0 = 0
    while n0 < want0 or len(preds) < want0 + 400:
        img = int(rng.randint(0, 64))
        o = gd[img][int(rng.randint(0, 10))]
        j = rng.normal(0, 6.0, 4) if rng.uniform() < 0.5 else rng.uniform(-60, 60, 4)
        label = o[4] if n0 < want0 else 1
        n0 += label == 0
        preds.append([img, o[0] + j[0], o[1] + j[1], o[2] + j[2], o[3] + j[3], 0., label])
    scores = np.unique(rng.uniform(0.01, 0.99, 2 * len(preds)).astype(np.float32))
    for p, s in zip(preds, rng.permutation(scores)[:len(preds)]):
        p[5] = float(s)
    preds = [[p[0]] + [float(np.float32(v)) for v in p[1:5]] + p[5:] for p in preds]
    case = vc.Case(gd, sorted(gd), preds, 2)
    vc.assert_distinct_scores(case)
    assert sum(p[6] == 0 for p in preds) == want0
    return case, {m07: vc.reference_table(case, 0.5, m07) for m07 in (False, True)}


def test_segment_longer_than_three_passes(long_case):
    case, want = long_case
    ev, _ = _device_eval(case, cap=256)
    for m07 in (False, True):
        assert 0.05 < want[m07][0, 4] < 0.95
        vc.assert_table(_c_entries(case, 0.5, m07)[0], want[m07], m07, 'long entries')
        vc.assert_table(ev.finish(0.5, m07), want[m07], m07, 'long DeviceEval')


def test_two_runs_give_the_same_bits(long_case):
    case, _ = long_case
    tables = []
    for _ in range(2):
        ev, _ = _device_eval(case, cap=256)
        tables.append([ev.finish(0.5, m07) for m07 in (False, True)])
    np.testing.assert_array_equal(tables[0], tables[1])
    np.testing.assert_array_equal(_c_entries(case, 0.5, False)[0], _c_entries(case, 0.5, False)[0])


def test_capacity_overflow_raises_and_writes_nothing_past_the_arena():
    import torch
    from yolov3_tensorflow_amd import _lib, framework as fw
    case = vc.random_case(3, images=10, classes=3)
    dev, R, guard = fw.default_device(), 50, 64
    assert len(case.preds) > R + 20
    big = (torch.full((R + guard, 4), -3., dtype=torch.float64, device=dev), torch.full((R + guard,), -3., dtype=torch.float64, device=dev),
           torch.full((R + guard,), -3, dtype=torch.int32, device=dev), torch.full((R + guard,), -3, dtype=torch.int32, device=dev))
    ev, rows = _device_eval(case, [case.image_ids[:4], case.image_ids[4:]], cap=200, capacity_rows=R, arena=tuple(t[:R] for t in big))
    with pytest.raises(_lib.Y3Error, match='did not fit'):
        ev.finish()
    assert ev._state.cpu().numpy().tolist() == [R, len(rows) - R]
    for t in big:
        assert (t[R:] == -3).all()
    np.testing.assert_array_equal(big[1][:R].cpu().numpy(), np.array([r[5] for r in rows[:R]], np.float64))
    assert (big[2][:R] >= 0).all()


def test_eval_script_with_and_without_map_on_device(tmp_path, capsys, isolated_graph):
    """eval.py end to end on a synthetic 6-image / 5-class set with random weights, host bookkeeping against
    --map_on_device true: the same per-class npos, nd, recall and precision, AP within the bound, the same printed lines."""
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd.utils import eval_utils
    sys.path.insert(0, os.path.dirname(HERE))
    import eval as eval_script
    common = eval_script_set(tmp_path)
    results, texts = {}, {}
    for on_device in ('false', 'true'):
        y3.reset_default_graph()
        results[on_device] = eval_script.main(common + ['--map_on_device', on_device])
        texts[on_device] = capsys.readouterr().out
    host, device = results['false'], results['true']
    assert len(host['val_preds']) > 50 and device['val_preds'] == [] and 'table' not in host
    with np.errstate(all='ignore'):
        want = np.array([[float(v) for v in eval_utils.voc_eval(host['gt_dict'], host['val_preds'], c)] for c in range(5)])
    capsys.readouterr()
    vc.assert_table(device['table'], want, False, 'eval.py')
    report = lambda text: [l for l in text.splitlines() if l.startswith(('Class ', 'final mAP', 'recall:', 'total_loss', 'mAP eval'))]
    assert len(report(texts['true'])) == 9 and report(texts['true']) == report(texts['false'])
