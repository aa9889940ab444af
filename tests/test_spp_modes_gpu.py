"""One whole train step with the features of the large-batch configuration on at once - the SPP architecture, the CIoU box
loss, LAMB, the weight moving average, the weight gradients on the second stream - against fp64, not only against itself:
tests/test_train_modes_sizes_gpu.py holds such steps to a fresh model's bit for bit, which leaves open whether the fresh step is
right.  256 x 256, bs = 4, f32, through test_spp_gpu._spp_step (data seeds 21 / 5, parameters seed 1).

The oracle is composed from what exists: spp_cases.SppMixin over iou_loss_cases' IouGraph (oracle.train_ref.TrainGraph with the
header's IoU box term), on the GPU's LeakyReLU branches and the GPU's pool argmax.  Every tolerance is imported from the test
that owns it:
    loss, gradients    test_spp_gpu.LOSS_RTOL / LOSS_ATOL / GRAD_TOL (tests/test_train_gpu.py::_step_matches_oracle's)
    variables, slots,  layerwise_cases.TOL of the tensor's max, one round, against layerwise_cases.evaluate on the GPU's own
    trust ratios       gradients (test_layerwise_update_gpu.test_apply_gradients_over_three_rounds_matches_the_chained_fp64_rule)
    shadows            ema_cases.bound around ema_cases.ema64
    moving statistics  1e-4 of the tensor's scale, test_spp_gpu._gate_against_fp64's

Preconditions, measured on the CPU with the oracle on its own branches (test_the_oracle_resolves_a_wrong_pool_backward prints
them): the ignore mask - no record's best IoU within test_train_gpu.OFF_SQUARE's 1e-4 of 0.5: the smallest distances on the
three scales are 2.4e-4, none (no image has a box on the middle scale) and 3.9e-3; the CIoU term's min / max - no object record
has a corner pair of its predicted and true boxes within iou_loss_cases.TIE_MARGIN = 1e-3 px: the closest pairs are 1.57 px and
2.47 px apart on the two scales with boxes."""
import numpy as np
import pytest
import torch

import ema_cases as E
import iou_loss_cases as IC
import layerwise_cases as LC
import spp_cases as sc
import test_spp_gpu as TSPP
from conftest import COCO_ANCHORS, blob_images
from test_conv_schedules_gpu import GUARD
from test_train_gpu import OFF_SQUARE, _conv_name, rel_err

BOX_LOSS, RULE, EMA_DECAY = 'ciou', 'lamb', 0.999
HEAD_CONV_2 = _conv_name(54) + '/weights'      # the kernel under the pool: its gradient passes through the pool backward


def graph_class():
    """class G(spp_cases.SppMixin, iou_loss_cases' IouGraph) with the box kind as an attribute (TrainGraph.compute_loss calls
    loss_layer without one) and the live tensors of the pool block kept for the guard"""
    class G(sc.SppMixin, IC._graph_class()):
        box_loss = BOX_LOSS
        pool_live = None
        corner_gaps = None      # a list: per scale, the smallest corner-pair distance over the object records

        def _spp(self, x):
            out = sc.SppMixin._spp(self, x)
            self.pool_live = (x, out)
            return out

        def loss_layer(self, fm, y_true, anchors, use_label_smooth=False, use_focal_loss=False):
            if self.corner_gaps is not None:
                yt = torch.as_tensor(np.asarray(y_true), dtype=self.dtype)
                q = IC.box_parts(self.decode(fm.detach(), yt, anchors), yt[..., 0:4])
                obj = yt[..., 4] != 0
                self.corner_gaps.append(float(q['corners'].abs().min(-1).values[obj].min()) if bool(obj.any()) else float('inf'))
            return super(G, self).loss_layer(fm, y_true, anchors, use_label_smooth, use_focal_loss, self.box_loss)
    return G


def _data():
    """test_spp_gpu._spp_step's defaults"""
    from oracle import train_ref
    return (sc.spp_params(80, seed=1), blob_images(21, 4, 256),
            train_ref.synthetic_targets(5, 4, [256, 256], 80, COCO_ANCHORS, max_boxes=4))


@pytest.mark.gpu
def test_one_spp_ciou_lamb_step_with_averaging_matches_fp64(isolated_graph):
    """Gradients (as backward left them: raw, no L2 term - weight_decay is LAMB's lambda - and unclipped) and the loss against the
    fp64 oracle; the updated variables, both slots, the direction left in the views and the trust ratios against the fp64 rule on
    the GPU's own gradients; the shadows against the fp64 moving average of the w the step stored; the moving statistics against
    the oracle's batch statistics.  See the module text for the tolerances and the preconditions; the two margins are asserted
    here on the oracle run that takes the GPU's branches.

    Measured on the MI355X (printed): gradients worst 3.2e-5, median 9.1e-6 over 225 tensors; against the fp64 rule, of the
    tensor's max: w 5.4e-8, the direction 3.1e-7, slot 0 1.1e-7, slot 1 2.5e-7, ratio 1.2e-7; the shadows 0.32 of their bound.
    With the bias corrections formed from the double betas instead of the float32 ones the kernel runs on (Trainer._apply_layerwise
    before this test) the direction and the ratios were 6.9e-6 and 6.7e-6 off, 3.4 tolerances."""
    import yolov3_tensorflow_amd as y3
    run = TSPP._spp_step(RULE, 'all', 'f32', True, box_loss=BOX_LOSS, ema_decay=EMA_DECAY)
    trainer, model, params, lr = run['trainer'], run['model'], run['params'], run['lr']
    assert model.wgrad_stream is True and model.spp and model.box_loss == BOX_LOSS and len(trainer.views) == 225
    # ---- the loss and the gradients ----
    g = graph_class()(params, 80, torch.float64, masks=run['masks'])
    g.pool_argmax, g.iou_margins, g.corner_gaps = run['argmax'], [], []
    loss = g.compute_loss(g.forward(run['x']), run['yts'], COCO_ANCHORS)
    names = [k for k, v in g.p.items() if v.requires_grad]
    ref = dict(zip(names, (t.numpy() for t in torch.autograd.grad(loss[0], [g.p[k] for k in names]))))
    print('smallest |best IoU - 0.5| per scale: %s ; smallest corner-pair distance per scale: %s px' % (g.iou_margins, g.corner_gaps))
    assert min(g.iou_margins) >= OFF_SQUARE['min_iou_margin'], g.iou_margins
    assert min(g.corner_gaps) >= IC.TIE_MARGIN, g.corner_gaps
    got_loss, want_loss = [float(v) for v in run['loss']], [float(v.detach()) for v in loss]
    assert got_loss[2] == 0.0 and want_loss[2] == 0.0      # (an IoU kind has no wh term)
    for a, b in zip(got_loss, want_loss):
        assert abs(a - b) <= TSPP.LOSS_RTOL * abs(b) + TSPP.LOSS_ATOL, (got_loss, want_loss)
    raw = {k: t.cpu().numpy() for k, t in run['raw_grads'].items()}
    assert set(raw) == set(ref)
    errs = {k: rel_err(raw[k], ref[k]) for k in ref}
    worst = max(errs, key=errs.get)
    print('spp/ciou/lamb/f32: gradient rel err vs the fp64 oracle on the GPU\'s branches and argmax: worst %.2e (%s), median %.2e '
          'over %d tensors' % (errs[worst], worst, float(np.median(list(errs.values()))), len(errs)))
    for k, e in errs.items():
        assert e < TSPP.GRAD_TOL, '%s: grad rel err %.3e' % (k, e)
    # ---- the rule, on the GPU's own gradients ----
    opt = trainer.opt
    assert opt.step == 1 and trainer.global_step == 1.0
    ema_step = trainer.ema_step_at(0.0)
    assert ema_step == E.step_at(EMA_DECAY, 0) == 1.0 - 1.0 / 10.0
    hp = LC.hyper(RULE, step=1, grad_scale=1.0, clip_norm=trainer.clip_norm, lr=lr, momentum=opt.momentum, beta1=opt.beta1,
                  beta2=opt.beta2, trust=opt.trust, eps=opt.epsilon, ema_step=ema_step)
    ratios = trainer.trust_ratios()
    shadows = trainer.ema_tensors()
    by_name = {v.op_name: v for v in y3.global_variables(scope='yolov3')}
    order = [v.op_name for v in trainer.order]
    got, want, worst_shadow = [], [], 0.0
    for k in order:
        kernel = k.endswith('/weights')
        w0 = np.asarray(params[k], np.float32)
        t = dict(w=w0, g=raw[k], s0=np.zeros_like(w0), s1=np.zeros_like(w0), wd=LC.F32(model.weight_decay) if kernel else 0.0,
                 flags=0 if kernel else LC.NO_ADAPT)
        want.append(LC.evaluate(RULE, t, hp))
        s0, s1 = opt.slots[k]
        got.append(dict(w=by_name[k].numpy(), g=trainer.views[k].cpu().numpy(), s0=s0.cpu().numpy(), s1=s1.cpu().numpy(),
                        ratio=np.float64(ratios[k])))
        assert (ratios[k] == 1.0) == (not kernel), (k, ratios[k])
        # the shadow started as a copy of the variable
        worst_shadow = max(worst_shadow, E.worst_ratio(shadows[k].cpu().numpy(), E.ema64(w0, got[-1]['w'], ema_step),
                                                       E.bound(w0, got[-1]['w'])))
    print('spp/ciou/lamb/f32: worst error / max|expected| against the fp64 rule: %s ; shadows %.3f of their bound'
          % (LC.fmt(LC.distance(got, want)), worst_shadow))
    LC.assert_close(got, want, 'spp/ciou/lamb')
    assert worst_shadow <= 1.0, worst_shadow
    # ---- the moving statistics ----
    for name, (mean, _, var_u) in g.batch_stats.items():
        for leaf, stat in (('moving_mean', mean), ('moving_variance', var_u)):
            k = '%s/BatchNorm/%s' % (name, leaf)
            new = (g.p[k] * 0.99 + stat * (1 - 0.99)).numpy()
            assert np.abs(by_name[k].numpy() - new).max() <= 1e-4 * max(np.abs(new).max(), 1e-6), k
    assert len(g.batch_stats) == 73


def test_the_oracle_resolves_a_wrong_pool_backward():
    """The guard, on the CPU with the oracle alone (its own branches, its own argmax; the GPU test's data): a pool block that
    routes the slot gradients in the order [5, 9, 13] instead of [13, 9, 5], and one without its identity term, must each move
    the gradient of head conv 2's kernel by at least GUARD (tests/test_conv_schedules_gpu.py: 10) times GRAD_TOL.  The wrong
    backward is the right one applied to d loss / d spp(x) with its slots exchanged, or with the last slot zeroed; the right one
    is checked against autograd's gradient of the whole graph.

    Measured: slots exchanged 9.50e-1 of the tensor's max (4,750 x GRAD_TOL), identity term dropped 4.52e-1 (2,261 x)."""
    params, x, yts = _data()
    g = graph_class()(params, 80, torch.float64)
    g.keep_trace = False
    g.iou_margins, g.corner_gaps = [], []
    loss = g.compute_loss(g.forward(x), yts, COCO_ANCHORS)
    print('oracle on its own branches: smallest |best IoU - 0.5| per scale %s ; smallest corner-pair distance per scale %s px'
          % (g.iou_margins, g.corner_gaps))
    assert min(g.iou_margins) >= OFF_SQUARE['min_iou_margin'] and min(g.corner_gaps) >= IC.TIE_MARGIN
    xin, pooled = g.pool_live
    kernel = g.p[HEAD_CONV_2]
    assert tuple(kernel.shape) == (1, 1, 1024, 512) and pooled.shape[1] == 4 * xin.shape[1] == 2048 and xin.shape[2:] == (8, 8)
    whole, dpooled = torch.autograd.grad(loss[0], [kernel, pooled], retain_graph=True)
    c = xin.shape[1]
    d13, d9, d5, did = (dpooled[:, j * c:(j + 1) * c] for j in range(4))

    def kernel_gradient(slots):
        dx, = torch.autograd.grad(pooled, xin, torch.cat(slots, 1), retain_graph=True)
        return torch.autograd.grad(xin, kernel, dx, retain_graph=True)[0].numpy()

    right = kernel_gradient([d13, d9, d5, did])
    assert rel_err(right, whole.numpy()) < 1e-12
    factors = {}
    for what, slots in (('slots exchanged', [d5, d9, d13, did]), ('identity term dropped', [d13, d9, d5, torch.zeros_like(did)])):
        e = rel_err(kernel_gradient(slots), right)
        factors[what] = e / TSPP.GRAD_TOL
        print('%s: %.2e of the tensor\'s max, %.0f x GRAD_TOL' % (what, e, factors[what]))
    for what, f in factors.items():
        assert f >= GUARD, (what, f)
