"""RCCL on the one GPU a box has: the train step through training.Trainer(process_group=WORLD) on a
world_size-1 `nccl` group launched under torch.distributed.run, with the bucket all-reduces FORCED (a one-rank group
would skip them).  This is the only RCCL evidence obtainable without a second GPU; the value semantics of two ranks are
covered by the gloo tests (tests/test_distributed_cpu.py, tests/test_data_parallel_gpu.py), the scaling curve by the
driver's 8-GPU run.

  (a) buckets are issued (asynchronous all-reduce works in flight) before backward has finished launching;
  (b) with ReduceOp.SUM the step equals the no-group step bit for bit (variables AND the flat gradient buffer);
  (c) stream ordering: with a pre-multiplied sum (factor 2) a one-rank all-reduce DOUBLES its bucket, so the result
      equals a no-group step whose clip/update kernel scales the gradients by 2 only if every all-reduce ran after the
      kernels that wrote its bucket and before mt_prepare_kernel read it — an ordering mistake between the process
      group's stream and the y3 context stream would leave a bucket undoubled (or doubled too late);
  (d) the same with update_vars that split layers and the weight gradients on backward's second stream, where a layer
      training only gamma / beta issues its `ready` edge next to a weight gradient still on that stream.  Timing-dependent
      (a race either shows or not); tests/test_train_gpu.py::test_every_ready_edge_follows_the_weight_gradients_it_covers
      is the deterministic form.
"""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_train_step_over_a_one_rank_rccl_group():
    out = tempfile.mkdtemp()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(HERE, 'workers', 'rccl_one_rank.py'), out]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors='replace')[-4000:]
    with open(os.path.join(out, 'meta.json')) as f:
        meta = json.load(f)
    assert meta['backend'] == 'nccl' and meta['world'] == 1
    m = meta['sum']
    # (a) whole-model gradients (248 MB) in 16 MiB buckets: most of them go out while backward is still running
    assert m['buckets'] >= 8 and m['issued_before_end'] >= m['buckets'] - 1, m
    assert m['works_in_flight'] == m['issued_before_end'], m
    # (b) SUM over one rank is the identity: bit-exact against the no-group step
    a, b = np.load(os.path.join(out, 'sum_group.npz')), np.load(os.path.join(out, 'sum_local.npz'))
    assert set(a.files) == set(b.files) and len(a.files) > 300
    for k in a.files:
        assert np.array_equal(a[k], b[k]), 'SUM all-reduce over one rank changed %s' % k
    # (c) the ordering check
    if not meta['premul']:
        pytest.fail('this RCCL build rejects the pre-multiplied sum (%s): the stream-ordering check did not run'
                    % meta.get('premul_error'))
    flat_sum = np.load(os.path.join(out, 'sum_local.npz'))['flat']
    plain = np.load(os.path.join(out, 'sum_local.npz'))
    # (the split step leaves most variables alone: its factor-2 effect is checked against its own no-group twin only)
    for tag, min_moved in (('premul', 200), ('premul_split', None)):
        assert tag in meta, '%s did not run' % tag
        a, b = np.load(os.path.join(out, '%s_group.npz' % tag)), np.load(os.path.join(out, '%s_local.npz' % tag))
        moved = 0
        for k in a.files:
            if k == 'flat':
                continue
            assert np.allclose(a[k], b[k], rtol=0, atol=1e-7 * max(1.0, float(np.abs(b[k]).max()))), \
                '%s all-reduce vs grad_scale=2: %s differs by %.3e' % (tag, k, float(np.abs(a[k] - b[k]).max()))
            moved += int(not np.array_equal(b[k], plain[k]))
        if min_moved is not None:
            assert moved > min_moved, 'the factor-2 step must differ from the plain step for the trained variables ' \
                                      '(%d did)' % moved
        # the issued buckets tile the trainable part of the buffer: [0, end) in order, nothing left out
        issued = meta[tag]['issued']
        assert issued and issued[0][0] == 0 and issued[-1][1] == meta[tag]['flat_end'], (tag, issued)
        assert all(p[1] == q[0] for p, q in zip(issued, issued[1:])), (tag, issued)
        assert np.abs(a['flat'][:issued[-1][1]]).max() > 0, tag
    assert np.isfinite(flat_sum).all()
