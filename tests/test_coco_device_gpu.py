"""GPU tests of the device COCO evaluator: y3_coco_match / y3_coco_ap / y3_coco_summary (include/yolo355.h) through
eval_utils.DeviceEval.finish_coco against eval_utils.coco_eval, held to the bounds of tests/test_coco_device_cpu.py (precision
and recall bit for bit; the twelve numbers within n * 2**-52), plus what only the kernels have: "taken" words in the LDS and in
the scratch, class lists longer than one pass of the AP kernel, an arena that is not full or overflows, real y3_nms output, and
run-to-run identity."""
import os
import sys

import numpy as np
import pytest

import coco_cases as cc
from device_eval_helpers import eval_script_set, nms_like

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _from_rows(case, spare=7, **kw):
    """The case's rows as float64 straight into an arena with `spare` rows to spare, in two pieces, in arrival order."""
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    p = case.preds
    ev = DeviceEval(case.gt_dict, case.image_ids, case.class_num, capacity_rows=len(p) + spare, **kw)
    for part in (p[:len(p) // 3], p[len(p) // 3:]):
        if part:
            ev.add_rows([r[0] for r in part], [r[1:5] for r in part], [r[5] for r in part], [r[6] for r in part])
    return ev


def _through_append(case, batch=5, cap=None, **kw):
    """The case's detections through y3_voc_append in the layout y3_nms leaves them in (slots past an image's count hold
    poison), image batches in image_ids order.  Returns the evaluator and the rows in the arena's order."""
    from collections import Counter
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils.eval_utils import DeviceEval
    cap = cap or max([1] + list(Counter(p[0] for p in case.preds if p[0] in case.image_ids).values()))
    ev = DeviceEval(case.gt_dict, case.image_ids, case.class_num, **kw)
    rows = []
    for b0 in range(0, len(case.image_ids), batch):
        ids = case.image_ids[b0:b0 + batch]
        dets, r = nms_like(case.preds, ids, cap, fw.default_device())
        ev.add(ids, dets)
        rows += r
    return ev, rows


def _is_fp32(case):
    return all(float(np.float32(v)) == v for p in case.preds for v in p[1:6])


@pytest.mark.parametrize('name', sorted(cc.corner_cases()))
def test_corner_cases_on_the_device(name):
    case = cc.corner_cases()[name]
    want = cc.reference(case)
    got = _from_rows(case).finish_coco(case.area_scale, return_curves=True)      # (the arena is not full)
    cc.assert_result(got, want, name)
    short = _from_rows(case, spare=0).finish_coco(case.area_scale)
    assert sorted(short) == ['per_class', 'stats']
    np.testing.assert_array_equal(short['stats'], got['stats'])
    np.testing.assert_array_equal(short['per_class'], got['per_class'])
    if _is_fp32(case):
        ev, rows = _through_append(case)
        cc.assert_result(ev.finish_coco(case.area_scale, return_curves=True), cc.reference(case._replace(preds=rows)), name + ' append')


@pytest.mark.parametrize('seed,images,classes', [(1, 12, 4), (2, 40, 5), (3, 6, 3)])
def test_random_sets(seed, images, classes):
    exact = cc.random_case(seed, images, classes, fp32=False)       # float64 rows straight into the arena
    case = cc.random_case(seed, images, classes, fp32=True)         # fp32 detections through y3_voc_append
    scales = {k: 0.4 + 0.35 * i for i, k in enumerate(case.image_ids)}
    cc.assert_result(_from_rows(exact).finish_coco(return_curves=True), cc.reference(exact), 'rows %d' % seed)
    ev, rows = _through_append(case, capacity_rows=len(case.preds) + 100)
    by_arrival = case._replace(preds=rows)
    cc.assert_result(ev.finish_coco(return_curves=True), cc.reference(by_arrival), 'append %d' % seed)
    cc.assert_result(ev.finish_coco(scales, return_curves=True), cc.reference(by_arrival._replace(area_scale=scales)), 'scaled %d' % seed)


def test_finish_and_finish_coco_on_one_evaluator():
    """Both read the arena and leave it alone: the VOC table is the same before and after finish_coco, and the COCO numbers the
    same before and after finish."""
    case = cc.random_case(1)
    ev, _ = _through_append(case)
    coco_first = ev.finish_coco(return_curves=True)
    table = ev.finish()
    coco_again = ev.finish_coco(return_curves=True)
    np.testing.assert_array_equal(ev.finish(), table)
    for key in coco_first:
        np.testing.assert_array_equal(coco_first[key], coco_again[key])
    ev2, _ = _through_append(case)
    np.testing.assert_array_equal(ev2.finish(), table)


@pytest.fixture(scope='module')
def long_case():
    from yolov3_tensorflow_amd import _lib
    case = cc.long_case(_lib.lib().y3_coco_ap_pass())
    return case, cc.reference(case)


def test_a_class_list_longer_than_two_passes(long_case):
    case, want = long_case
    assert 0.02 < want['stats'][0] < 0.9
    ev, rows = _through_append(case, batch=16)
    assert rows == case.preds
    cc.assert_result(ev.finish_coco(return_curves=True), want, 'long')


def test_two_runs_give_the_same_bits(long_case):
    case, _ = long_case
    runs = [_through_append(case, batch=16)[0].finish_coco(return_curves=True) for _ in range(2)]
    for key in ('precision', 'recall', 'stats', 'per_class'):
        np.testing.assert_array_equal(runs[0][key], runs[1][key])


def test_more_objects_in_an_image_than_the_lds_holds_words_for():
    from yolov3_tensorflow_amd import _lib
    case = cc.many_objects_case(_lib.lib().y3_coco_lds_objects() + 8)
    assert len(case.gt_dict[1]) > _lib.lib().y3_coco_lds_objects() and _is_fp32(case)
    want = cc.reference(case)
    cc.assert_result(_from_rows(case).finish_coco(return_curves=True), want, 'many objects')
    ev, rows = _through_append(case)
    assert rows == case.preds
    cc.assert_result(ev.finish_coco(return_curves=True), want, 'many objects append')


def test_capacity_overflow_raises():
    from yolov3_tensorflow_amd import _lib
    case = cc.random_case(3, 6, 3)
    assert len(case.preds) > 50
    ev, rows = _through_append(case, capacity_rows=40)
    with pytest.raises(_lib.Y3Error, match='did not fit'):
        ev.finish_coco()
    assert ev._state.cpu().numpy().tolist() == [40, len(rows) - 40]


def test_real_nms_output_through_add():
    """Detections as y3_nms leaves them (gpu_nms_batched, lazy): DeviceEval.add + finish_coco against coco_eval on the rows
    get_preds_batch builds from the same detections."""
    import torch
    from yolov3_tensorflow_amd import framework as fw
    from yolov3_tensorflow_amd.utils import eval_utils
    from yolov3_tensorflow_amd.utils.nms_utils import gpu_nms_batched
    rng = np.random.RandomState(9)
    n, B, C = 6, 300, 4
    gts, boxes, scores = {}, np.zeros((n, B, 4), np.float32), np.zeros((n, B, C), np.float32)
    for i in range(n):
        objs = []
        for _ in range(int(rng.randint(1, 7))):
            x0, y0 = rng.uniform(0, 250, 2)
            side = float(rng.choice([rng.uniform(10, 30), rng.uniform(34, 90), rng.uniform(100, 150)]))
            objs.append([x0, y0, x0 + side, y0 + side, int(rng.randint(0, C))])
        gts[10 + i] = objs
        for b in range(B):
            o = objs[b % len(objs)]
            if b < B // 2:
                boxes[i, b] = np.array(o[:4]) + rng.normal(0, 0.05 * (o[2] - o[0]), 4)
                scores[i, b, o[4]] = rng.uniform(0.05, 0.95)
            else:
                x0, y0 = rng.uniform(0, 250, 2)
                boxes[i, b] = [x0, y0, x0 + rng.uniform(10, 150), y0 + rng.uniform(10, 150)]
                scores[i, b, int(rng.randint(0, C))] = rng.uniform(0.05, 0.6)
    dev = fw.default_device()
    dets = gpu_nms_batched(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), C, 30, 0.1, 0.45, lazy=True)
    ids = list(gts)
    ev = eval_utils.DeviceEval(gts, ids, C)
    ev.add(ids, dets)
    got = ev.finish_coco(return_curves=True)
    rows = eval_utils.get_preds_batch(ids, dets)
    assert 60 < len(rows) <= n * C * 30
    want = eval_utils.coco_eval(gts, rows, C)
    cc.assert_result(got, want, 'real nms')
    assert 0.05 < want['stats'][0] < 0.95 and (want['stats'] > -1).all()


def test_eval_script_with_and_without_coco_metric(tmp_path, capsys, isolated_graph):
    """eval.py end to end on a synthetic 6-image / 5-class set with random weights: with --coco_metric true the twelve numbers of
    --map_on_device true and false agree within the bound and twelve lines follow the VOC report; with the flag off the
    output is what it is without the option."""
    import yolov3_tensorflow_amd as y3
    sys.path.insert(0, os.path.dirname(HERE))
    import eval as eval_script
    common = eval_script_set(tmp_path)
    results, texts = {}, {}
    for key, extra in (('host', ['--coco_metric', 'true']), ('device', ['--coco_metric', 'true', '--map_on_device', 'true']),
                       ('off', ['--coco_metric', 'false']), ('plain', [])):
        y3.reset_default_graph()
        results[key] = eval_script.main(common + extra)
        texts[key] = capsys.readouterr().out
    host, device = results['host']['coco'], results['device']['coco']
    assert len(results['host']['val_preds']) > 50 and 'coco' not in results['off'] and 'coco' not in results['plain']
    assert sorted(host) == ['per_class', 'precision', 'recall', 'stats'] and sorted(device) == ['per_class', 'stats']
    cc.assert_result(device, host, 'eval.py')
    assert texts['off'] == texts['plain']
    coco_lines = [l for l in texts['host'].splitlines() if l.startswith('Average ')]
    assert len(coco_lines) == 12 and texts['host'] == texts['plain'] + '\n'.join(coco_lines) + '\n'
    assert [l for l in texts['device'].splitlines() if l.startswith('Average ')] == coco_lines
    assert coco_lines[0].startswith('Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ')
