#!/usr/bin/env python
"""Throughput of one training step (BASELINE configs[3]: 416x416, bs=64 per GPU, SGD) on synthetic batches.

    python tools/train_bench.py [--batch 64] [--steps 5] [--optimizer sgd] [--head-only] [--box_loss giou]

--sync_bn measures what synchronised batch norm (training.Trainer(sync_bn=True)) costs on ONE GPU: a one-rank `nccl` group
with the 144 collectives per step forced (as tests/test_rccl_gpu.py forces the gradient buckets), rounds of --steps steps
alternating with and without the hook in one job, written to profiles/sync_bn_rate.txt.  It says nothing about the cost
with more than one RCCL rank, where each collective also crosses xGMI and waits for the slowest rank.
"""
import argparse
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_y_true(n, size, class_num, anchors, seed, device):
    """Device-side stand-in for process_box output: a few object cells per image per scale."""
    import torch
    g = torch.Generator(device='cpu').manual_seed(seed)
    out = []
    for s, a0 in ((32, 6), (16, 3), (8, 0)):
        gsz = size // s
        y = torch.zeros((n, gsz, gsz, 3, 6 + class_num))
        y[..., -1] = 1.0
        for i in range(n):
            for _ in range(3):
                cy, cx, k = (int(torch.randint(0, gsz, (1,), generator=g)), int(torch.randint(0, gsz, (1,), generator=g)),
                             int(torch.randint(0, 3, (1,), generator=g)))
                w, h = float(anchors[a0 + k][0]), float(anchors[a0 + k][1])
                y[i, cy, cx, k, 0:4] = torch.tensor([(cx + 0.5) * s, (cy + 0.5) * s, w, h])
                y[i, cy, cx, k, 4] = 1.0
                y[i, cy, cx, k, 5 + int(torch.randint(0, class_num, (1,), generator=g))] = 1.0
        out.append(y.to(device))
    return out


def sync_bn_ab(a, model, upd, x, yt):
    """Rounds of a.steps steps, alternately without and with the batch-norm exchange hook (one Trainer, one workspace)."""
    import tempfile
    import torch
    import torch.distributed as dist
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('nccl', init_method='file://' + os.path.join(tempfile.mkdtemp(), 'init'), rank=0, world_size=1)
    # (the weight-gradient stream fixed on: the 'auto' calibration would spend its seven steps inside the first rounds)
    trainer = training.Trainer(model, config_optimizer(a.optimizer, 1e-4), update_vars=upd, process_group=dist.group.WORLD,
                               wgrad_stream=True, sync_bn=True)
    ms = {False: [], True: []}
    for on in (False, True):      # warm both arms (RCCL sets its communicator up in the first collective)
        trainer.bn_sync.force = on
        for _ in range(2):
            trainer.step(x, yt)
    for _ in range(a.rounds):
        for on in (False, True):
            trainer.bn_sync.force = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                trainer.step(x, yt)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / a.steps * 1e3)
    calls = len(trainer.bn_sync.calls)
    dist.destroy_process_group()
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ['# synchronised batch norm on ONE GPU: a one-rank nccl group, the collectives forced (tools/train_bench.py --sync_bn)',
             '# train step [%s] batch %d @%d, %s%s, wgrad_stream on; %d rounds x %d steps per arm, alternating in one job'
             % (a.precision, a.batch, a.size, a.optimizer, ' head-only' if a.head_only else '', a.rounds, a.steps),
             '# hook calls per step: %d' % calls,
             'without ms/step: %s  median %.2f' % (' '.join('%.2f' % v for v in ms[False]), med(ms[False])),
             'with    ms/step: %s  median %.2f' % (' '.join('%.2f' % v for v in ms[True]), med(ms[True])),
             'difference of the medians: %+.2f ms/step (%+.2f%%)' % (med(ms[True]) - med(ms[False]),
                                                                   100 * (med(ms[True]) / med(ms[False]) - 1)),
             '# one rank: no xGMI traffic and no waiting for a slower rank - not the cost at world > 1']
    print('\n'.join(lines))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--optimizer', default='sgd')
    ap.add_argument('--head-only', action='store_true')
    ap.add_argument('--precision', default='f32', choices=['f32', 'f32_wino', 'f32_bf16x6', 'f32_bf16x3', 'bf16'],
                    help='the train mode (training._TRAIN_DTYPES): bf16 = mixed precision on the bf16 matrix pipe')
    ap.add_argument('--box_loss', default='mse', choices=['mse', 'giou', 'diou', 'ciou'],
                    help="the loss's box term (yolov3.box_loss): the reference's squared errors, or one IoU term")
    ap.add_argument('--ignore_thresh', type=float, default=0.5,
                    help="the loss's ignore threshold (yolov3.ignore_thresh; the reference: 0.5, darknet: 0.7)")
    ap.add_argument('--obj_iou_ratio', type=float, default=0.0,
                    help='r of the objectness target (1 - r) + r * IoU of a positive (yolov3.obj_iou_ratio; 0: target 1)')
    ap.add_argument('--ema_decay', type=float, default=0,
                    help='above 0: keep the weight moving average in the update kernel (training.Trainer(ema_decay=...))')
    ap.add_argument('--spp', action='store_true', help='the YOLOv3-SPP architecture (yolov3.spp): 76 convs and the pooling block')
    ap.add_argument('--sync_bn', action='store_true', help='A/B of synchronised batch norm over a one-rank nccl group')
    ap.add_argument('--rounds', type=int, default=4, help='--sync_bn: rounds per arm')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sync_bn_rate.txt'))
    return ap


def main():
    a = build_parser().parse_args()
    import torch
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    import bench
    model = y3.yolov3(80, bench.ANCHORS, batch_norm_decay=0.99)
    model.compute_dtype = a.precision
    model.spp = a.spp
    model.box_loss = a.box_loss
    model.ignore_thresh, model.obj_iou_ratio = a.ignore_thresh, a.obj_iou_ratio
    x =torch.rand((a.batch, a.size, a.size, 3), device='cuda')
    yt = synthetic_y_true(a.batch, a.size, 80, bench.ANCHORS, 0, 'cuda')
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros((1, 64, 64, 3), device='cuda'))
        bench.random_init(1)
        upd = None
        if a.head_only:
            upd = [v for v in y3.global_variables(scope='yolov3') if v.op_name.startswith('yolov3/yolov3_head')]
        if a.sync_bn:
            return sync_bn_ab(a, model, upd, x, yt)
        trainer = training.Trainer(model, config_optimizer(a.optimizer, 1e-4), update_vars=upd, ema_decay=a.ema_decay)
        for _ in range(2):
            loss = trainer.step(x, yt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = trainer.step(x, yt)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
    # 3x the forward's direct-convolution FLOPs: bench.conv_flops for the default architecture, as ever; it knows that head's
    # divisors only, so the SPP net's come from the net's own tensor table (the same formula)
    topo = model._train['topo']
    if a.spp:
        flops = 3 * sum(2.0 * l['k'] ** 2 * l['cin'] * l['cout'] * (a.size // topo.tensors[l['dst']]['sdiv']) ** 2 * a.batch
                        for l in topo.layers)
    else:
        flops = 3 * bench.conv_flops([(l['k'], l['stride'], l['cin'], l['cout'], l['bn']) for l in topo.layers],
                                     a.batch, a.size, a.size).sum()
    print('train step [%s%s, box_loss %s%s]: batch %d @%d, %s%s: %.1f ms/step, %.1f images/s, %.1f TFLOP/s (3x forward FLOPs), loss %.3f, peak mem %.1f GB'
          % (a.precision, ', spp' if a.spp else '', a.box_loss,
             (', ignore_thresh %g, obj_iou_ratio %g' % (a.ignore_thresh, a.obj_iou_ratio)
              if (a.ignore_thresh, a.obj_iou_ratio) != (0.5, 0.0) else '') +
             (', ema_decay %g' % a.ema_decay if a.ema_decay else ''), a.batch, a.size, a.optimizer, ' head-only' if a.head_only else '', dt * 1e3, a.batch / dt,
             flops / dt / 1e12, float(loss[0]), torch.cuda.max_memory_allocated() / 1e9))


if __name__ == '__main__':
    main()
