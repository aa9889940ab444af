"""Synchronised batch norm over two ranks on DEVICE tensors: `training.Trainer(process_group=..., sync_bn=True)`.
Transport as in tests/test_data_parallel_gpu.py: `nccl` (RCCL) with one device per rank where two GPUs are visible, `gloo` on
the shared cuda:0 otherwise; the process group has a timeout, so a rank that fails ends its peer instead of hanging it.

Rank r holds 2 images at 96 x 96.  Checked:
  * both ranks end a step with bit-identical variables, the BN moving statistics included;
  * the averaged gradients (rank 0's flat buffer after the exchange, times grad_scale) are those of ONE step on the
    concatenated 4-image batch: every tensor within GRAD_TOL = 2e-4 (tests/test_train_gpu.py) of oracle/train_ref.train_step
    in fp64, evaluated on the LeakyReLU branches the GPU took, as that test does; the mean of the two ranks' losses is the
    oracle's loss to 1e-4;
  * the same two ranks WITHOUT sync_bn miss that tolerance for at least one BN gamma (so the test resolves the feature).
    Chosen seeds, checked on the CPU beforehand with train_ref alone: the mean of the gradients of the two 2-image shards
    against the gradient of the 4-image batch differs by 2.8e-2 (best gamma) to 2.3 (worst) of the tensor's max - two to
    four orders above 2e-4;
  * an uneven split, forward only: ranks with 1 and 3 images leave the stem's moving statistics of a single-process
    4-image forward (the row count travels with the sums)."""
import datetime
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import COCO_ANCHORS, blob_images

pytestmark = pytest.mark.gpu

N, SIZE, DECAY = 2, 96, 0.9
GRAD_TOL = 2e-4          # tests/test_train_gpu.py
STEM = 'yolov3/darknet53_body/Conv/BatchNorm/'


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-12))


def _conv_name(i):
    sub, j = ('darknet53_body', i) if i < 52 else ('yolov3_head', i - 52)
    return 'yolov3/%s/%s' % (sub, 'Conv' if j == 0 else 'Conv_%d' % j)


def _params():
    from oracle import yolo_ref
    return yolo_ref.synthetic_params(80, seed=3)


def _setup():
    import yolov3_tensorflow_amd as y3
    params = _params()
    y3.reset_default_graph()
    model = y3.yolov3(80, COCO_ANCHORS, batch_norm_decay=DECAY, weight_decay=5e-4)
    model.compute_dtype = 'f32_wino'
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    for v in y3.global_variables(scope='yolov3'):
        v.assign(params[v.op_name])
    return y3, model


def _data(rank):
    from oracle import train_ref
    return blob_images(40 + rank, N, SIZE), train_ref.synthetic_targets(50 + rank, N, [SIZE, SIZE], 80, COCO_ANCHORS, max_boxes=3)


def _step(tag, rank, sync_bn, out_dir):
    """forward / loss / backward / exchange on this rank's shard; saves the averaged gradients, the loss, the branches taken
    and the variables after the update"""
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    y3, model = _setup()
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), process_group=dist.group.WORLD, sync_bn=sync_bn)
    trainer.capture = []
    x, yts = _data(rank)
    with y3.variable_scope('yolov3'):
        fms = model.forward(x, is_training=True)
        loss = training.compute_loss(model, fms, yts)
        trainer.backward()
        trainer.exchange.finish()
        grads = {k: (v * trainer.exchange.grad_scale).cpu().numpy() for k, v in trainer.views.items()}
        masks = {}
        for rec in trainer.capture:
            if rec['z'] is not None:
                masks[_conv_name(rec['layer'])] = ((rec['z'] * rec['stats'][2] + rec['stats'][3]) > 0).permute(0, 3, 1, 2).cpu()
        trainer.capture = None
        calls = list(trainer.bn_sync.calls) if trainer.bn_sync is not None else None
        trainer.apply_gradients()
    torch.cuda.synchronize()
    torch.save(dict(grads=grads, masks=masks, loss=[float(v) for v in loss], calls=calls,
                    state={v.op_name: v.numpy() for v in y3.global_variables(scope='yolov3')}),
               os.path.join(out_dir, '%s%d.pt' % (tag, rank)))


def _worker(rank, world, init_file, out_dir):
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    import yolov3_tensorflow_amd as y3_
    backend, device = ('nccl', rank) if torch.cuda.device_count() >= 2 else ('gloo', 0)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(device)
    y3_.set_default_device('cuda:%d' % device)
    dist.init_process_group(backend, init_method='file://' + init_file, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=120))
    _step('sync', rank, True, out_dir)
    _step('plain', rank, False, out_dir)
    # uneven split, forward only: rank 0 holds image 0, rank 1 images 1..3 of the 4-image batch
    x4 = np.concatenate([_data(0)[0], _data(1)[0]])
    y3, model = _setup()
    training.Trainer(model, config_optimizer('sgd', 1e-3), process_group=dist.group.WORLD, sync_bn=True)
    with y3.variable_scope('yolov3'):
        model.forward(x4[:1] if rank == 0 else x4[1:], is_training=True)
    torch.cuda.synchronize()
    stem = {k: v.numpy() for k in ('moving_mean', 'moving_variance') for v in y3.global_variables(scope='yolov3')
            if v.op_name == STEM + k}
    dist.barrier()
    if rank == 0:      # ... and the single-process 4-image forward they must agree with
        y3, model = _setup()
        with y3.variable_scope('yolov3'):
            model.forward(x4, is_training=True)
        torch.cuda.synchronize()
        stem.update({'whole_' + k: v.numpy() for k in ('moving_mean', 'moving_variance')
                     for v in y3.global_variables(scope='yolov3') if v.op_name == STEM + k})
    torch.save(dict(stem=stem, backend=backend), os.path.join(out_dir, 'uneven%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def ranks():
    d = tempfile.mkdtemp()
    mp.spawn(_worker, args=(2, os.path.join(d, 'init'), d), nprocs=2, join=True)
    load = lambda name: torch.load(os.path.join(d, name), weights_only=False)
    out = {tag: [load('%s%d.pt' % (tag, r)) for r in range(2)] for tag in ('sync', 'plain', 'uneven')}
    print('two-rank sync-BN steps ran on backend %s' % out['uneven'][0]['backend'])
    return out


_ORACLE = {}


def _oracle(tag, runs):
    """fp64 step on the concatenated batch, on the branches the two ranks took (no L2 term, no clip: the raw gradients)"""
    if tag not in _ORACLE:
        from oracle import train_ref
        d0, d1 = _data(0), _data(1)
        masks = {k: torch.cat([runs[0]['masks'][k], runs[1]['masks'][k]]) for k in runs[0]['masks']}
        _ORACLE[tag] = train_ref.train_step(_params(), np.concatenate([d0[0], d1[0]]),
                                            [np.concatenate([d0[1][i], d1[1][i]]) for i in range(3)], COCO_ANCHORS, class_num=80,
                                            optimizer='sgd', lr=1e-3, weight_decay=0.0, bn_decay=DECAY, clip=1e30,
                                            dtype=torch.float64, masks=masks)
    return _ORACLE[tag]


def test_both_ranks_end_with_identical_variables_moving_statistics_included(ranks):
    r0, r1 = ranks['sync']
    assert r0['calls'] == r1['calls'] and len(r0['calls']) == 144
    moving = [k for k in r0['state'] if '/moving_' in k]
    assert len(moving) == 144 and set(r0['state']) == set(r1['state'])
    for k in r0['state']:
        np.testing.assert_array_equal(r0['state'][k], r1['state'][k], err_msg=k)
    # (without the switch they differ: tests/test_data_parallel_gpu.py asserts it, and so does this run)
    p0, p1 = ranks['plain']
    assert np.abs(p0['state'][STEM + 'moving_mean'] - p1['state'][STEM + 'moving_mean']).max() > 0
    params = _params()
    assert np.abs(r0['state'][STEM + 'moving_mean'] - params[STEM + 'moving_mean']).max() > 0


def test_averaged_gradients_and_loss_are_those_of_the_four_image_batch(ranks):
    r0, r1 = ranks['sync']
    ref = _oracle('sync', ranks['sync'])
    assert set(r0['grads']) == set(ref['grads'])
    errs = {k: rel_err(r0['grads'][k], g) for k, g in ref['grads'].items()}
    worst = max(errs, key=errs.get)
    print('sync-BN, two ranks vs the fp64 4-image step: worst gradient rel err %.2e (%s), median %.2e over %d tensors'
          % (errs[worst], worst, float(np.median(list(errs.values()))), len(errs)))
    for k, e in errs.items():
        assert e < GRAD_TOL, '%s: grad rel err %.3e' % (k, e)
    for a, b, want in zip(r0['loss'], r1['loss'], ref['loss']):
        assert abs(0.5 * (a + b) - want) <= 1e-4 * abs(want) + 1e-6, (r0['loss'], r1['loss'], ref['loss'])


def test_without_sync_bn_the_same_ranks_miss_the_four_image_gradients(ranks):
    r0 = ranks['plain'][0]
    assert r0['calls'] is None
    ref = _oracle('plain', ranks['plain'])
    errs = {k: rel_err(r0['grads'][k], g) for k, g in ref['grads'].items() if k.endswith('/BatchNorm/gamma')}
    print('no sync-BN: gamma gradient rel err vs the 4-image step: min %.2e, max %.2e' % (min(errs.values()), max(errs.values())))
    assert max(errs.values()) > GRAD_TOL


def test_an_uneven_split_leaves_the_statistics_of_the_whole_batch(ranks):
    u0, u1 = ranks['uneven']
    for k in ('moving_mean', 'moving_variance'):
        np.testing.assert_array_equal(u0['stem'][k], u1['stem'][k])
        np.testing.assert_allclose(u0['stem'][k], u0['stem']['whole_' + k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert np.abs(u0['stem']['moving_mean'] - _params()[STEM + 'moving_mean']).max() > 0
