"""CPU tests of the host side of synchronised batch norm: `distributed.BnSync` on CPU tensors over a world-2 `gloo` group
(the object `training.Trainer(sync_bn=True)` hands to y3_net_train_set_bn_sync), its no-op forms, the `--sync_bn` option of
train.py, and that a Trainer without a process group installs no hook."""
import ctypes
import datetime
import os
import subprocess
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = [(0, 0, 65), (1, 0, 129), (3, 0, 2049), (3, 1, 2049), (1, 1, 129), (0, 1, 65)]      # (layer, phase, doubles)


def _worker(rank, world, init_file, out_dir):
    from yolov3_tensorflow_amd import distributed
    dist.init_process_group('gloo', init_method='file://' + init_file, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    sync = distributed.BnSync(None)
    assert sync.world == world and sync.active and sync.buf.dtype == torch.float64
    assert sync.buf.numel() == distributed.BN_SYNC_DOUBLES == 2 * 1024 + 1
    got = []
    sync.begin()
    for layer, phase, doubles in CALLS:
        c = (doubles - 1) // 2
        sync.buf.fill_(-1.0)
        sync.buf[:2 * c] = torch.arange(2 * c, dtype=torch.float64) * (rank + 1) + layer + phase      # the column sums
        sync.buf[2 * c] = 10.0 + 5 * rank                                                         # this rank's row count
        assert sync(layer, phase, doubles) == 0
        got.append(sync.buf.clone())
    calls = list(sync.calls)
    # an exception inside the hook is kept, not thrown: the hook is called from C
    sync.exchange = lambda doubles: (_ for _ in ()).throw(ValueError('no such group'))
    rc = sync(9, 0, 65)
    kept = repr(sync.error)
    try:
        sync.raise_error()
        raised = None
    except ValueError as e:
        raised = str(e)
    torch.save(dict(got=got, calls=calls, rc=rc, kept=kept, raised=raised, cleared=sync.error is None),
               os.path.join(out_dir, 'r%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_bn_sync_sums_buffer_and_count_over_two_gloo_ranks():
    d = tempfile.mkdtemp()
    mp.spawn(_worker, args=(2, os.path.join(d, 'init'), d), nprocs=2, join=True)
    r0, r1 = torch.load(os.path.join(d, 'r0.pt')), torch.load(os.path.join(d, 'r1.pt'))
    for r in (r0, r1):
        assert r['calls'] == [(l, p) for l, p, _ in CALLS]          # in the order given
        assert r['rc'] != 0 and 'no such group' in r['kept'] and r['raised'] == 'no such group' and r['cleared']
    for (layer, phase, doubles), a, b in zip(CALLS, r0['got'], r1['got']):
        assert torch.equal(a, b)
        c = (doubles - 1) // 2
        assert torch.equal(a[:2 * c], torch.arange(2 * c, dtype=torch.float64) * 3 + 2 * (layer + phase))
        assert float(a[2 * c]) == 25.0                               # the count travels with the sums
        assert torch.equal(a[doubles:], torch.full((2049 - doubles,), -1.0, dtype=torch.float64))      # nothing past `doubles`


def test_bn_sync_without_a_group_is_a_no_op():
    from yolov3_tensorflow_amd import distributed
    assert not dist.is_initialized()
    sync = distributed.BnSync()
    assert sync.world == 1 and not sync.active
    sync.buf[:5] = torch.arange(5, dtype=torch.float64)
    sync.begin()
    assert sync(3, 0, 5) == 0 and sync(3, 1, 5) == 0
    assert sync.calls == [(3, 0), (3, 1)] and sync.error is None
    assert torch.equal(sync.buf[:5], torch.arange(5, dtype=torch.float64))
    sync.begin()
    assert sync.calls == []
    # forced without a group: the collective cannot run, and the hook says so with a status, not an exception
    sync.force = True
    assert sync.active and sync(0, 0, 5) != 0 and sync.error is not None


def test_train_script_has_the_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert '--sync_bn' in text and '144' in ' '.join(text.split())
    sys.path.insert(0, ROOT)
    try:
        import train
        assert train.build_parser().parse_args([]).sync_bn is False
        assert train.build_parser().parse_args(['--sync_bn', 'true']).sync_bn is True
    finally:
        sys.path.remove(ROOT)


def test_trainer_with_sync_bn_but_no_group_installs_no_hook():
    import numpy as np
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    anchors = np.arange(18, dtype=np.float32).reshape(9, 2) + 1
    model = y3.yolov3(80, anchors)
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), sync_bn=True)
    assert trainer.bn_sync is model.bn_sync and not trainer.bn_sync.active
    training._train_net(model, ctypes.c_void_p())        # (host only: a net without a context)
    assert model._train['bn_sync_cb'] is None
    assert training.Trainer(model, config_optimizer('sgd', 1e-3)).bn_sync is None and model.bn_sync is None
