"""Training path (reference train.py:72-115): yolov3.forward(is_training=True) with batch-statistics BN,
compute_loss, backward, per-tensor clip, optimizer update, optional data-parallel gradient all-reduce.

Python here only sequences C-ABI calls over caller-owned device buffers (torch = allocator + process group);
every number is produced by a HIP kernel of csrc/y3_train.hip, y3_wgrad.hip or y3_conv.hip.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import distributed
from . import framework as fw

BN_EPS = 1e-5      # model.py:37
CLIP_NORM = 100.0  # train.py:113-114


class Optimizer(object):
    """Hyper-parameters + slot variables of one of the four update rules the reference can select
    (utils/misc_utils.py:151-161; TF1 definitions), or of one of the layer-wise rules for large global
    batches (include/yolo355.h, "Layer-wise update rules"): 'adamw' (decoupled weight decay), 'lars' (momentum with a
    per-tensor trust ratio; `trust` is its coefficient) and 'lamb' (Adam with one).  For those three the model's
    weight_decay is the rule's lambda, not an L2 term in the gradient."""

    KINDS = ('sgd', 'momentum', 'adam', 'rmsprop', 'adamw', 'lars', 'lamb')      # in ABI order
    LAYERWISE = KINDS[4:]                                                       # y3_layerwise_update_multi's
    _EPSILON = dict(adam=1e-8, adamw=1e-8, lamb=1e-6)

    def __init__(self, kind, learning_rate, momentum=0.9, decay=0.9, beta1=0.9, beta2=0.999, epsilon=None, trust=0.001):
        if kind not in self.KINDS:
            raise ValueError('Unsupported optimizer type!')
        self.kind = kind
        self.learning_rate = learning_rate   # float, or a callable global_step -> float
        self.momentum = momentum
        self.decay = decay
        self.beta1, self.beta2 = beta1, beta2
        self.epsilon = epsilon if epsilon is not None else self._EPSILON.get(kind, 1e-10)
        self.trust = trust
        self.slots = {}                      # variable op_name -> (slot0, slot1) device tensors
        self.step = 0                        # number of apply_gradients calls (adam's t)

    def lr_at(self, global_step):
        return float(self.learning_rate(global_step)) if callable(self.learning_rate) else float(self.learning_rate)

    def _slots_for(self, var):
        s = self.slots.get(var.op_name)
        if s is None:
            z = lambda: torch.zeros_like(var.tensor)
            if self.kind == 'sgd':
                s = (None, None)
            elif self.kind in ('momentum', 'lars'):
                s = (z(), None)
            elif self.kind in ('adam', 'adamw', 'lamb'):
                s = (z(), z())
            else:                            # rmsprop: ms initialised to ones, mom to zeros (TF1)
                s = (torch.ones_like(var.tensor), z())
            self.slots[var.op_name] = s
        return s


# --------------------------------------------------------------------------------------------------------
# graph topology (queried from the C++ launch plan: one source of truth)
# --------------------------------------------------------------------------------------------------------
def _arch(model):
    """The Y3_ARCH_* code of the model: 1 (YOLOv3-SPP) with model.spp set, else 0."""
    return 1 if model.spp else 0


class _Topology(object):
    def __init__(self, class_num, arch=0):
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.y3_net_create_arch(None, int(class_num), int(arch), ctypes.byref(h)))
        self.layers = []
        ci = lambda: ctypes.c_int()
        for i in range(L.y3_net_num_layers(h)):
            k, s, cin, cout, bn = ci(), ci(), ci(), ci(), ci()
            _lib.check(L.y3_net_layer_info(h, i, *[ctypes.byref(v) for v in (k, s, cin, cout, bn)]))
            src, up, resid, dst, act = ci(), ci(), ci(), ci(), ci()
            _lib.check(L.y3_net_layer_graph(h, i, *[ctypes.byref(v) for v in (src, up, resid, dst, act)]))
            self.layers.append(dict(k=k.value, stride=s.value, cin=cin.value, cout=cout.value, bn=bool(bn.value),
                                    src=src.value, up=up.value, resid=resid.value, dst=dst.value, act=act.value))
        self.tensors = []
        for t in range(L.y3_net_num_tensors(h)):
            c, sd, ext = ci(), ci(), ci()
            _lib.check(L.y3_net_tensor_info(h, t, ctypes.byref(c), ctypes.byref(sd), ctypes.byref(ext)))
            self.tensors.append(dict(c=c.value, sdiv=sd.value, ext=ext.value))
        L.y3_net_destroy(h)


def _scratch(state, key, nbytes, device):
    t = state.setdefault('scratch', {}).get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        state['scratch'][key] = t
    return t


def _train_state(model):
    st = getattr(model, '_train', None)
    if st is None:
        st = dict(topo=_Topology(model.class_num, _arch(model)), net=None, arch=_arch(model))
        model._train = st
    if st['arch'] != _arch(model):
        raise ValueError("model.spp must be set before the first training forward (the train net is built for it)")
    return st


# y3_net dtype codes of the compute modes the train step accepts (bf16: mixed precision, bf16 tensors and products with fp32
# statistics, gradients, variables and optimizer; include/yolo355.h, train-step block)
_TRAIN_DTYPES = {'f32': 0, 'bf16': 1, 'f32_bf16x6': 2, 'f32_bf16x3': 3, 'f32_wino': 4}


def _train_net(model, ctx, dev=None):
    """The y3_net handle the train step runs on (one per model; its dtype follows model.compute_dtype at every call: the
    dtype only selects kernels, the state a forward leaves is the same in every mode)."""
    st = _train_state(model)
    L = _lib.lib()
    if st['net'] is None or st.get('net_ctx') != ctx.value:
        h = ctypes.c_void_p()
        _lib.check(L.y3_net_create_arch(ctx, int(model.class_num), st['arch'], ctypes.byref(h)))
        st['net'], st['net_ctx'] = h, ctx.value
    mode = getattr(model, 'compute_dtype', 'f32')
    if mode not in _TRAIN_DTYPES:
        raise ValueError("training needs compute_dtype in %s (got %r)" % (sorted(_TRAIN_DTYPES), mode))
    if st.get('net_dtype') != mode:
        _lib.check(L.y3_net_set_dtype(st['net'], _TRAIN_DTYPES[mode]))
        st['net_dtype'] = mode
    # backward's second stream (include/yolo355.h: y3_net_train_set_wgrad_stream): on unless model.wgrad_stream is False
    # True: on a low-priority stream the library creates; False: off; a torch.cuda.Stream: on that stream
    want = getattr(model, 'wgrad_stream', False)
    handle = (want.cuda_stream if isinstance(want, torch.cuda.Stream) else 1) if want else None       # 1 = Y3_OWN_STREAM
    key = (handle, st['net'].value)
    if st.get('wgrad_key') != key:
        if isinstance(want, torch.cuda.Stream):
            st['side_stream'] = want        # (kept alive)
        _lib.check(L.y3_net_train_set_wgrad_stream(st['net'], ctypes.c_void_p(handle) if handle else None))
        st['wgrad_key'] = key
        st['ws_shape'] = None            # (the allocation sequence of backward changes with it)
    _set_box_loss(model, st)
    _set_conf_rule(model, st)
    # synchronised batch norm (include/yolo355.h: y3_net_train_set_bn_sync): the distributed.BnSync a Trainer(sync_bn=True)
    # left on the model, installed while it is active
    sync = getattr(model, 'bn_sync', None)
    sync = sync if sync is not None and sync.active else None
    key = (id(sync) if sync is not None else None, st['net'].value)
    if st.get('bn_sync_key') != key:
        if sync is None:
            _lib.check(L.y3_net_train_set_bn_sync(st['net'], _lib.BnSyncFn(), None, None, 0))
            st['bn_sync_cb'] = None
        else:
            if sync.buf.device.type != 'cuda':
                sync.buf = sync.buf.to(dev if dev is not None else fw.default_device())
            cb = _lib.BnSyncFn(lambda user, layer, phase, doubles: sync(layer, phase, doubles))
            _lib.check(L.y3_net_train_set_bn_sync(st['net'], cb, None, fw.ptr(sync.buf),
                                                  ctypes.c_size_t(sync.buf.numel() * sync.buf.element_size())))
            st['bn_sync_cb'] = (cb, sync)        # (kept alive while the net may call it)
        st['bn_sync_key'] = key
    return st['net']


def _box_kind(model):
    """The Y3_BOX_* kind of model.box_loss ('mse' for a model object from before the attribute)."""
    from .model import BOX_LOSSES
    name = getattr(model, 'box_loss', 'mse')
    if name not in BOX_LOSSES:
        raise ValueError("box_loss must be one of %s (got %r)" % (sorted(BOX_LOSSES), name))
    return BOX_LOSSES[name]


def _set_box_loss(model, st):
    """model.box_loss on the train net (include/yolo355.h: y3_net_train_set_box_loss), whenever either has changed."""
    key = (_box_kind(model), st['net'].value)
    if st.get('box_loss_key') != key:
        _lib.check(_lib.lib().y3_net_train_set_box_loss(st['net'], key[0]))
        st['box_loss_key'] = key


def _conf_rule(model):
    """(ignore_thresh, obj_iou_ratio) of the model ((0.5, 0) for a model object from before the attributes)."""
    return float(getattr(model, 'ignore_thresh', 0.5)), float(getattr(model, 'obj_iou_ratio', 0.0))


def _set_conf_rule(model, st):
    """model.ignore_thresh / obj_iou_ratio on the train net (include/yolo355.h: y3_net_train_set_conf_rule), whenever either
    has changed."""
    key = _conf_rule(model) + (st['net'].value,)
    if st.get('conf_rule_key') != key:
        _lib.check(_lib.lib().y3_net_train_set_conf_rule(st['net'], key[0], key[1]))
        st['conf_rule_key'] = key


def _checked(model, rc):
    """_lib.check for the train-step entries: an exception the batch-norm exchange hook caught comes first."""
    sync = getattr(model, 'bn_sync', None)
    if sync is not None:
        sync.raise_error()
    _lib.check(rc)


def _var_table(layer_vars, offsets=None, layer_ends=None):
    """ctypes array of y3_train_var for the 75 layers.  offsets: {op_name: element offset into the flat gradient buffer}
    for the trainable variables (None: every trainable variable, in gradient_layout's order - used to size the workspace);
    layer_ends: {layer index: offset just after that layer's gradients} (the `ready` hook's argument)."""
    if offsets is None:
        _, offsets, layer_ends, _ = gradient_layout(layer_vars)
    arr = (_lib.TrainVar * len(layer_vars))()
    keep = []
    off = lambda v: int(offsets.get(v.op_name, -1)) if v is not None else -1
    ptr = lambda v: v.tensor.data_ptr() if v is not None else None
    for i, (wvar, bnv, bias) in enumerate(layer_vars):
        g, b, mm, mv = bnv if bnv is not None else (None, None, None, None)
        arr[i] = _lib.TrainVar(ptr(wvar), ptr(g), ptr(b), ptr(mm), ptr(mv), ptr(bias), off(wvar), off(g), off(b), off(bias),
                               int((layer_ends or {}).get(i, -1)))
        keep.append([v.tensor for v in (wvar, g, b, mm, mv, bias) if v is not None])
    return arr, keep


def _opts(model):
    anc = np.ascontiguousarray(np.asarray(model.anchors, np.float32).reshape(9, 2))
    o = _lib.TrainOpts(float(model.batch_norm_decay), 1 if model.use_label_smooth else 0, 1 if model.use_focal_loss else 0,
                       anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return o, anc


# --------------------------------------------------------------------------------------------------------
# forward in training mode
# --------------------------------------------------------------------------------------------------------
def _prepare(model, x):
    """Everything a training forward needs before the library call: the train net in the model's mode, the variables (created
    on first use, in the reference's order), their table, the workspace (sized for every variable trainable: an upper bound
    for any update_vars subset, checked for layer-splitting ones by tests/test_train_workspace_cpu.py), the options."""
    st = _train_state(model)
    topo = st['topo']
    L = _lib.lib()
    dev = x.device
    net = _train_net(model, fw.context(dev), dev)
    scope = fw.current_scope_name()
    layer_vars = model._ensure_variables(scope, [(l['k'], l['stride'], l['cin'], l['cout'], l['bn'])
                                                 for l in topo.layers])
    n, h, w, _ = x.shape
    key = tuple(t.tensor.data_ptr() for lv in layer_vars for t in ((lv[0],) + tuple(lv[1] or ()) + ((lv[2],) if lv[2] is not None else ())))
    if st.get('vars_key') != key:
        st['vars_all'], st['vars_keep'] = _var_table(layer_vars)
        st['vars_key'] = key
    ws_key = (n, h, w, str(dev), model.compute_dtype)      # the allocation sequence depends on the net's dtype too
    if st.get('ws_shape') != ws_key:
        need = L.y3_net_train_workspace_bytes(net, st['vars_all'], n, h, w)
        if need == 0:
            _lib.check(_lib.Y3_EINVAL)
        ws = st.get('ws')
        if ws is None or ws.numel() < need or ws.device != dev:
            st['ws'] = None              # (free the old one first)
            st['ws'] = torch.empty(need, dtype=torch.uint8, device=dev)
        st['ws_shape'] = ws_key
    st.update(layer_vars=layer_vars, batch=n, x=x, have_loss=False)
    return st, net, layer_vars


def _after_forward(model, st, fm_ptrs):
    """Bookkeeping after a training forward: the moving statistics changed in place; the feature maps are views of the
    workspace."""
    for wvar, bnv, bias in st['layer_vars']:
        if bnv is not None:        # updated in place: the folded inference parameters must be rebuilt
            bnv[2].touch()
            bnv[3].touch()
    ws, x = st['ws'], st['x']
    n, h, w, _ = x.shape
    det = 3 * (5 + model.class_num)
    fms = []
    for p, s in zip(fm_ptrs, (32, 16, 8)):
        o = p - ws.data_ptr()
        fms.append(ws[o:o + n * (h // s) * (w // s) * det * 4].view(torch.float32).view(n, h // s, w // s, det))
    st.update(fms=fms, fm_ptrs=list(fm_ptrs))
    return fms


def forward_train(model, x):
    """yolov3.forward(inputs, is_training=True): BN normalises with batch statistics in ALL 72 BN layers and
    updates the moving statistics (decay = model.batch_norm_decay); activations are kept for backward.
    ONE library call (y3_net_train_forward); the feature maps are views into the step's workspace."""
    st, net, layer_vars = _prepare(model, x)
    n, h, w, _ = x.shape
    opts, anc = _opts(model)
    fm = [ctypes.c_void_p() for _ in range(3)]
    if getattr(model, 'bn_sync', None) is not None:
        model.bn_sync.begin()
    _checked(model, _lib.lib().y3_net_train_forward(net, st['vars_all'], fw.ptr(x), n, h, w, ctypes.byref(opts), fw.ptr(st['ws']),
                                                    ctypes.c_size_t(st['ws'].numel()), *[ctypes.byref(p) for p in fm]))
    fms = _after_forward(model, st, [p.value for p in fm])
    return fms[0], fms[1], fms[2]


# --------------------------------------------------------------------------------------------------------
# loss (model.py:192-365)
# --------------------------------------------------------------------------------------------------------
def _loss_one_scale(model, fm, y_true, anchors, loss4, accumulate, grad):
    L = _lib.lib()
    fm = fw.as_device_f32(fm)
    y_true = fw.as_device_f32(y_true)
    n, gh, gw, ch = fm.shape
    C = int(model.class_num)
    if ch != 3 * (5 + C):
        raise ValueError("feature map has %d channels, expected %d" % (ch, 3 * (5 + C)))
    if tuple(y_true.shape) != (n, gh, gw, 3, 6 + C):
        raise ValueError("y_true shape %s does not match the feature map (expected %s)" %
                         (tuple(y_true.shape), (n, gh, gw, 3, 6 + C)))
    if model.img_size is None:
        raise ValueError("loss needs img_size: call forward() first")
    st = _train_state(model)
    sc = _scratch(st, 'loss', L.y3_loss_scratch_bytes(n, gh, gw), fm.device)
    anc = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(3, 2))
    ignore_thresh, obj_iou_ratio = _conf_rule(model)
    _lib.check(L.y3_loss_layer_conf(fw.context(fm.device), fw.ptr(fm), fw.ptr(y_true), n, gh, gw, C,
                                    int(model.img_size[0]), int(model.img_size[1]),
                                    anc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    1 if model.use_label_smooth else 0, 1 if model.use_focal_loss else 0, _box_kind(model),
                                    ignore_thresh, obj_iou_ratio, 1 if accumulate else 0, fw.ptr(loss4), fw.ptr(grad),
                                    int(grad.shape[-1]), fw.ptr(sc), ctypes.c_size_t(sc.numel())))


def loss_layer(model, feature_map_i, y_true, anchors):
    """reference model.py:192-304: returns (xy_loss, wh_loss, conf_loss, class_loss) device scalars.  With model.box_loss an
    IoU kind, xy_loss is the IoU box term and wh_loss is 0 (include/yolo355.h: y3_loss_layer_box)."""
    fm = fw.as_device_f32(feature_map_i)
    loss4 = torch.zeros(4, dtype=torch.float32, device=fm.device)
    grad = torch.zeros(tuple(fm.shape[:3]) + (fm.shape[3],), dtype=torch.float32, device=fm.device)
    _loss_one_scale(model, fm, y_true, anchors, loss4, False, grad)
    return loss4[0], loss4[1], loss4[2], loss4[3]


def compute_loss(model, y_pred, y_true):
    """reference model.py:348-365: [total, xy, wh, conf, class] over the three scales (anchors [6:9], [3:6],
    [0:3]).  When y_pred are the feature maps of the last forward(is_training=True) this is ONE library call
    (y3_net_train_loss) that also leaves d(total)/d(feature_map_i) in the step's workspace for the backward pass; any other
    feature maps (validation: forward(is_training=False)) take the per-scale entry point."""
    st = _train_state(model)
    L = _lib.lib()
    if st.get('fm_ptrs') is not None and [fw.as_device_f32(f).data_ptr() for f in y_pred] == st['fm_ptrs']:
        dev = st['fms'][0].device
        yt = [fw.as_device_f32(y) for y in y_true]
        for f, y in zip(st['fms'], yt):
            if tuple(y.shape) != tuple(f.shape[:3]) + (3, 6 + int(model.class_num)):
                raise ValueError("y_true shape %s does not match the feature map %s" % (tuple(y.shape), tuple(f.shape)))
        opts, anc = _opts(model)
        _set_box_loss(model, st)         # (the attributes may have changed since the forward)
        _set_conf_rule(model, st)
        loss5 = torch.empty(5, dtype=torch.float32, device=dev)
        _lib.check(L.y3_net_train_loss(st['net'], fw.ptr(yt[0]), fw.ptr(yt[1]), fw.ptr(yt[2]), ctypes.byref(opts),
                                       fw.ptr(loss5)))
        st['have_loss'] = True
        return [loss5[0], loss5[1], loss5[2], loss5[3], loss5[4]]
    anchors = np.asarray(model.anchors, np.float32).reshape(9, 2)
    groups = [anchors[6:9], anchors[3:6], anchors[0:3]]
    dev = fw.as_device_f32(y_pred[0]).device
    loss4 = torch.zeros(4, dtype=torch.float32, device=dev)
    det_pad = ((3 * (5 + model.class_num) + 31) // 32) * 32
    grads = []
    for i in range(3):
        fm = fw.as_device_f32(y_pred[i])
        g = torch.zeros(tuple(fm.shape[:3]) + (det_pad,), dtype=torch.float32, device=dev)   # pad lanes stay 0
        _loss_one_scale(model, fm, y_true[i], groups[i], loss4, i > 0, g)
        grads.append(g)
    st['fm_grads'] = grads       # (test hook: d total / d feature_map_i of this stand-alone evaluation)
    total = loss4.sum()
    return [total, loss4[0], loss4[1], loss4[2], loss4[3]]


def box_iou(pred_boxes, valid_true_boxes):
    """reference model.py:307-345: pred_boxes [g,g,3,4] (cx,cy,w,h), valid_true_boxes [V,4] -> iou [g,g,3,V].
    (Inside compute_loss the same arithmetic is fused into the loss kernel.)"""
    pb = fw.as_device_f32(pred_boxes)
    tb = fw.as_device_f32(valid_true_boxes).reshape(-1, 4)
    if pb.shape[-1] != 4:
        raise ValueError("pred_boxes must end in 4 (cx, cy, w, h)")
    v = int(tb.shape[0])
    out = torch.empty(tuple(pb.shape[:-1]) + (v,), dtype=torch.float32, device=pb.device)
    if v == 0 or pb.numel() == 0:
        return out
    _lib.check(_lib.lib().y3_box_iou(fw.context(pb.device), fw.ptr(pb), pb.numel() // 4, fw.ptr(tb), v, fw.ptr(out)))
    return out


# --------------------------------------------------------------------------------------------------------
# backward + update
# --------------------------------------------------------------------------------------------------------
def gradient_layout(layer_vars, trainable=lambda v: v.trainable):
    """Layout of the flat gradient buffer: the variables in the order backward PRODUCES their gradients (last layer
    first; inside a layer gamma, beta / bias, then the kernel), every view 16-byte aligned.  Pure host arithmetic over
    objects with .op_name / .shape (no device needed).
    Returns (order, offsets {op_name: element offset}, layer_ends {layer index: element offset just after that layer's
    gradients} (layers with a trainable variable only; increasing as the layer index decreases), total elements)."""
    order, offs, ends, total = [], {}, {}, 0
    layer_vars = list(layer_vars)
    for li in range(len(layer_vars) - 1, -1, -1):
        wvar, bnv, bias = layer_vars[li]
        vs = (list(bnv[:2]) if bnv is not None else [bias]) + [wvar]
        vs = [v for v in vs if trainable(v)]
        for v in vs:
            numel = 1
            for d in v.shape:
                numel *= int(d)
            offs[v.op_name] = total
            total += (numel + 3) // 4 * 4
            order.append(v)
        if vs:
            ends[li] = total
    return order, offs, ends, total


class Trainer(object):
    """One object = the train op of train.py:105-115: gradients of loss[0] + l2_loss w.r.t. update_vars,
    per-tensor clip_by_norm(100), optimizer.apply_gradients; with torch.distributed initialised, gradients
    are summed over ranks — RCCL all-reduce of the flat gradient buffer in buckets, issued in the order backward
    produces them and overlapped with the rest of backward (distributed.GradientExchange) — and averaged (the 1/world
    factor is folded into the clip/update kernel) before clipping.

    ema_decay in (0, 1) keeps a moving average of every updated variable (include/yolo355.h, "Weight moving average":
    tf.train.ExponentialMovingAverage(ema_decay, num_updates=global_step) with zero_debias=False; ema_warmup=False drops
    the num_updates ramp).  The update kernel writes the averages (y3_clip_update_multi_ema: no launch is added);
    `averaged()` puts them into the variables for validation and saving.  None or 0: off, and the step is the one without
    the argument, launch for launch.  Data-parallel ranks exchange nothing for it: every rank applies the same update to
    the same weights, so identical weights give identical averages."""

    def __init__(self, model, optimizer, update_vars=None, clip_norm=CLIP_NORM, process_group=None,
                 global_step=0.0, bucket_bytes=distributed.DEFAULT_BUCKET_BYTES, wgrad_stream='auto', sync_bn=False,
                 ema_decay=None, ema_warmup=True):
        self.model, self.opt = model, optimizer
        self.ema_decay = float(ema_decay) if ema_decay else None
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ValueError('ema_decay must lie in (0, 1), or be None / 0 for no averaging (got %r)' % (ema_decay,))
        self.ema_warmup = bool(ema_warmup)
        self.ema = None          # {op_name: the average of that variable} once the shadows exist (see _alloc_ema)
        self._ema_pending = {}   # averages a checkpoint handed over before the shadows existed
        self._averaged = False   # inside averaged(): the variables hold the averages, self.ema the raw values
        # Synchronised batch norm (distributed.BnSync; off by default): every BN layer normalises with the statistics of the
        # GLOBAL batch and every rank keeps the same moving statistics, so an N-rank step is the single-GPU step at N times
        # the batch (given equal local batch sizes).  Costs two small collectives per BN layer and step.  True, or a BnSync
        # of the caller's; the hook is installed only while that object is active - a group of more than one rank, or its
        # `force` test switch - and serves step() and the split forward(is_training=True) / compute_loss / backward() path.
        self.bn_sync = None
        if sync_bn:
            self.bn_sync = sync_bn if isinstance(sync_bn, distributed.BnSync) else distributed.BnSync(process_group)
        if self.bn_sync is not None or getattr(model, 'bn_sync', None) is not None:
            model.bn_sync = self.bn_sync        # (where forward(is_training=True), which has no Trainer, finds it)
        # backward's weight gradients on a second stream (include/yolo355.h: y3_net_train_set_wgrad_stream): True / False /
        # a torch.cuda.Stream / 'auto'.  Every result is bit-identical either way; only the step time differs - and by how
        # much depends on which hardware queue the second stream lands on (with many streams alive in the process it can
        # share the main stream's: 96 ms per bs=64 step instead of 79.6 against 81 on one stream,
        # profiles/r06_wgrad_stream_ab.txt).  'auto' therefore MEASURES: steps 3-4 with it, steps 6-7 without (hipEvents
        # around the step, one host synchronisation each), and keeps the faster; `wgrad_choice` tells which.
        self.wgrad_stream = wgrad_stream
        self.wgrad_choice = None if wgrad_stream == 'auto' else wgrad_stream
        self._calib = dict(step=0, on=[], off=[]) if wgrad_stream == 'auto' else None
        self.update_names = None if update_vars is None else set(v.op_name for v in update_vars)
        self.clip_norm = float(clip_norm)
        self.pg = process_group
        self.bucket_bytes = int(bucket_bytes)
        self.global_step = float(global_step)
        self.flat = None
        self.views = None
        self.exchange = None
        self.capture = None      # test hook: a list that backward() fills with each BN layer's (z, stats)

    def _trainable(self, var):
        return var.trainable and (self.update_names is None or var.op_name in self.update_names)

    def _alloc_grads(self, layer_vars, dev):
        if self.flat is not None:
            return
        order, offs, ends, total = gradient_layout(layer_vars, self._trainable)
        self.flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self.views = {v.op_name: self.flat[offs[v.op_name]:offs[v.op_name] + v.tensor.numel()].view(v.tensor.shape)
                      for v in order}
        self.order = order
        self.offsets = offs
        self.layer_ends = ends
        self.exchange = distributed.GradientExchange(self.flat, sorted(ends.values()) or [total], self.pg,
                                                     self.bucket_bytes)
        self._alloc_ema()

    # ---- moving average of the weights ---------------------------------------------------------------------------------
    def ema_step_at(self, global_step):
        """1 - d_t of the step taken at `global_step` (its value before the step increments it), in double:
        d_t = min(ema_decay, (1 + t) / (10 + t)) with warm-up, else ema_decay.  Pure host arithmetic."""
        if self.ema_decay is None:
            raise RuntimeError('this Trainer keeps no moving average (ema_decay is off)')
        t = float(global_step)
        d = min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay
        return 1.0 - d

    def _alloc_ema(self):
        """The shadows of self.order: each starts as a copy of its variable, or with the value a checkpoint handed over."""
        if self.ema_decay is None or self.ema is not None:
            return
        self.ema = {}
        for v in self.order:
            s = v.tensor.detach().clone()
            stored = self._ema_pending.pop(v.op_name, None)
            if stored is not None and tuple(stored.shape) == tuple(s.shape):
                s.copy_(torch.as_tensor(np.ascontiguousarray(stored, dtype=np.float32)))
            self.ema[v.op_name] = s
        self._ema_pending = {}

    def ema_assign(self, op_name, value):
        """Set the average of one variable (Saver.restore).  Before the shadows exist the value is kept and becomes the
        shadow's start value; a name the step does not update, or another shape, is ignored."""
        if self.ema_decay is None:
            return
        if self.ema is None:
            self._ema_pending[op_name] = np.array(value, dtype=np.float32)
            return
        t = self.ema_tensors().get(op_name)
        if t is not None and tuple(t.shape) == tuple(np.shape(value)):
            t.copy_(torch.as_tensor(np.ascontiguousarray(value, dtype=np.float32)))

    def ema_tensors(self):
        """{op_name: tensor holding that variable's AVERAGE}, inside and outside averaged() ({} while there are none)."""
        if self.ema is None:
            return {}
        return {v.op_name: v.tensor for v in self.order} if self._averaged else dict(self.ema)

    def raw_tensors(self):
        """{op_name: tensor holding the raw iterate} of the averaged variables."""
        if self.ema is None:
            return {}
        return dict(self.ema) if self._averaged else {v.op_name: v.tensor for v in self.order}

    def averaged(self):
        """Context manager: inside it every updated variable holds its average (validation, best-model files); on exit the
        raw values are back, bit for bit.  The tensors are swapped, not copied, and every variable is touch()ed so the
        packed-weight caches follow.  step(), backward() and apply_gradients() raise inside it.  Without averaging (or
        before the first step created the shadows) the context changes nothing."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            if self._averaged:
                raise RuntimeError('averaged() is already active')
            swap = self.ema is not None
            if swap:
                self._swap_ema()
            try:
                yield self
            finally:
                if swap:
                    self._swap_ema()
        return ctx()

    def _swap_ema(self):
        for v in self.order:
            v.tensor, self.ema[v.op_name] = self.ema[v.op_name], v.tensor
            v.touch()
        self._averaged = not self._averaged

    def _no_update_while_averaged(self, what):
        if self._averaged:
            raise RuntimeError('%s inside Trainer.averaged(): the variables hold their averages' % what)

    def _vars(self, layer_vars, dev):
        self._alloc_grads(layer_vars, dev)
        key = tuple(v.tensor.data_ptr() for v in self.order) + tuple(
            t.tensor.data_ptr() for lv in layer_vars for t in (lv[1][2:] if lv[1] is not None else ()))
        if getattr(self, '_vars_key', None) != key:
            self._vars_arr, self._vars_keep = _var_table(layer_vars, self.offsets, self.layer_ends)
            self._vars_key = key
        return self._vars_arr

    def _ready_cb(self):
        if getattr(self, '_cb', None) is None:
            self._cb = _lib.GradReadyFn(lambda user, edge: self.exchange.ready(int(edge)))
        return self._cb

    def _fill_capture(self, st):
        """Test hook: views of the tensors that fix each BN layer's LeakyReLU branch (z and the folded scale / shift)."""
        L = _lib.lib()
        topo, ws, n = st['topo'], st['ws'], st['batch']
        h, w = st['x'].shape[1:3]
        for i in range(len(topo.layers) - 1, -1, -1):
            l = topo.layers[i]
            zo, so = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(L.y3_net_train_saved(st['net'], i, ctypes.byref(zo), ctypes.byref(so)))
            if not l['bn']:
                self.capture.append(dict(layer=i, z=None, stats=None))
                continue
            sd = topo.tensors[l['dst']]['sdiv']
            cout = l['cout']
            zt, ze = (torch.bfloat16, 2) if L.y3_net_train_saved_type(st['net'], i) == 1 else (torch.float32, 4)
            z = ws[zo.value:zo.value + n * (h // sd) * (w // sd) * cout * ze].view(zt).view(n, h // sd, w // sd, cout)
            stats = ws[so.value:so.value + 4 * cout * 4].view(torch.float32).view(4, cout)
            self.capture.append(dict(layer=i, z=z, stats=stats))

    def backward(self):
        """train.py:112 compute_gradients: ONE library call (y3_net_train_backward) walks the graph backwards and writes every
        trainable variable's gradient into the flat buffer; the `ready` hook issues the gradient buckets as they complete."""
        self._no_update_while_averaged('backward()')
        st = _train_state(self.model)
        if not st.get('have_loss') or st.get('fms') is None:
            raise RuntimeError('backward needs forward(is_training=True) and compute_loss first')
        dev = st['fms'][0].device
        net = _train_net(self.model, fw.context(dev), dev)         # (the mode may have changed since the forward)
        arr = self._vars(st['layer_vars'], dev)
        self.exchange.begin()
        _checked(self.model, _lib.lib().y3_net_train_backward(net, arr, fw.ptr(self.flat), self._ready_cb(), None))
        if self.capture is not None:
            self._fill_capture(st)

    def _param_descs(self):
        """Host array of y3_param_desc for self.order (rebuilt when a variable's storage or a slot changed)."""
        sig = tuple((v.tensor.data_ptr(),) + tuple(0 if s is None else s.data_ptr() for s in self.opt._slots_for(v))
                    for v in self.order)
        if self.ema is not None:
            sig += tuple(self.ema[v.op_name].data_ptr() for v in self.order)
        if getattr(self, '_descs_sig', None) != sig:
            arr = (_lib.ParamDesc * len(self.order))()
            keep = []
            for i, v in enumerate(self.order):
                g = self.views[v.op_name]
                s0, s1 = self.opt._slots_for(v)
                kernel = v.op_name.endswith('/weights')
                wd = float(self.model.weight_decay) if kernel else 0.0
                # the layer-wise rules adapt the conv kernels only: gamma, beta and biases take ratio 1 (the old entry
                # points ignore the word)
                arr[i] = _lib.ParamDesc(v.tensor.data_ptr(), g.data_ptr(), 0 if s0 is None else s0.data_ptr(),
                                        0 if s1 is None else s1.data_ptr(), v.tensor.numel(), wd,
                                        0 if kernel else _lib.Y3_PARAM_NO_ADAPT)
                keep.append((v.tensor, s0, s1))
            self._descs, self._descs_keep, self._descs_sig = arr, keep, sig
            if self.ema is not None:        # the HOST array of shadow pointers of y3_clip_update_multi_ema, in self.order
                self._ema_arr = (ctypes.c_void_p * len(self.order))(*[self.ema[v.op_name].data_ptr() for v in self.order])
        return self._descs, self._descs_keep

    def apply_gradients(self):
        """all-reduce (mean over ranks) -> + weight_decay*w on conv kernels -> clip_by_norm -> update.
        adamw / lars / lamb: all-reduce -> clip_by_norm -> the rule, with weight_decay as its lambda on the conv kernels."""
        self._no_update_while_averaged('apply_gradients()')
        if self.opt.kind in Optimizer.LAYERWISE and os.environ.get('Y3_TRAIN_PER_TENSOR_UPDATE') == '1':
            raise RuntimeError("Y3_TRAIN_PER_TENSOR_UPDATE=1 runs one y3_clip_update per variable, which knows the kinds "
                               "%s only: '%s' needs every tensor's norms and goes through y3_layerwise_update_multi"
                               % (', '.join(Optimizer.KINDS[:4]), self.opt.kind))
        L = _lib.lib()
        dev = self.flat.device
        ctx = fw.context(dev)
        ema_step = None if self.ema is None else ctypes.c_float(self.ema_step_at(self.global_step))
        self.exchange.finish()      # buckets not yet issued by backward + join the asynchronous ones
        world = self.exchange.world
        self.opt.step += 1
        lr = self.opt.lr_at(self.global_step)
        kind = Optimizer.KINDS.index(self.opt.kind)
        if self.opt.kind == 'adam':
            t = self.opt.step
            lr = lr * np.sqrt(1.0 - self.opt.beta2 ** t) / (1.0 - self.opt.beta1 ** t)
        decay = self.opt.beta1 if self.opt.kind == 'adam' else self.opt.decay
        st = _train_state(self.model)
        if self.opt.kind in Optimizer.LAYERWISE:
            self._apply_layerwise(L, ctx, st, dev, kind, lr, world, ema_step)
            for v in self.order:
                v.touch()
            self.global_step += 1.0
            return
        if os.environ.get('Y3_TRAIN_PER_TENSOR_UPDATE') == '1':     # experiment hook: one y3_clip_update per variable
            sc = _scratch(st, 'opt', L.y3_optimizer_scratch_bytes(), dev)
            for v in self.order:
                s0, s1 = self.opt._slots_for(v)
                wd = float(self.model.weight_decay) if v.op_name.endswith('/weights') else 0.0
                _lib.check(L.y3_clip_update(ctx, kind, fw.ptr(v.tensor), fw.ptr(self.views[v.op_name]), fw.ptr(s0),
                                            fw.ptr(s1), v.tensor.numel(), ctypes.c_float(wd), ctypes.c_float(1.0 / world),
                                            ctypes.c_float(self.clip_norm), ctypes.c_float(lr),
                                            ctypes.c_float(self.opt.momentum), ctypes.c_float(decay),
                                            ctypes.c_float(self.opt.beta2), ctypes.c_float(self.opt.epsilon), fw.ptr(sc)))
                if ema_step is not None:
                    _lib.check(L.y3_ema_update(ctx, fw.ptr(self.ema[v.op_name]), fw.ptr(v.tensor), v.tensor.numel(), ema_step))
                v.touch()
            self.global_step += 1.0
            return
        # ONE multi-tensor call (three launches) for every (gradient, variable) pair of train.py:112-115
        descs, keep = self._param_descs()
        hp = (ctypes.c_float(1.0 / world), ctypes.c_float(self.clip_norm), ctypes.c_float(lr), ctypes.c_float(self.opt.momentum),
              ctypes.c_float(decay), ctypes.c_float(self.opt.beta2), ctypes.c_float(self.opt.epsilon))
        if ema_step is None:
            nbytes = L.y3_clip_update_multi_scratch_bytes(descs, len(self.order))
            sc = _scratch(st, 'opt_multi', nbytes, dev)
            _lib.check(L.y3_clip_update_multi(ctx, kind, descs, len(self.order), *(hp + (fw.ptr(sc), ctypes.c_size_t(sc.numel())))))
        else:       # the same three launches; the third also moves every shadow towards the w it stores
            nbytes = L.y3_clip_update_multi_ema_scratch_bytes(descs, len(self.order))
            sc = _scratch(st, 'opt_multi', nbytes, dev)
            _lib.check(L.y3_clip_update_multi_ema(ctx, kind, descs, len(self.order),
                                                  *(hp + (self._ema_arr, ema_step, fw.ptr(sc), ctypes.c_size_t(sc.numel())))))
        for v in self.order:
            v.touch()
        self.global_step += 1.0

    def _apply_layerwise(self, L, ctx, st, dev, kind, lr, world, ema_step):
        """adamw / lars / lamb: ONE y3_layerwise_update_multi call (three launches, lamb five) for every pair; the step's
        ratios stay on the device for trust_ratios()."""
        # the bias corrections are formed in double FROM THE FLOAT32 BETAS, the ones the kernel's m and v run on: from
        # the double 0.999 (float32: 0.99900001287) 1 - beta2^t is 1.3e-5 off at t = 1, and v * bias2 is then not gh^2
        t, b1, b2 = self.opt.step, float(np.float32(self.opt.beta1)), float(np.float32(self.opt.beta2))
        adaptive = self.opt.kind != 'lars'
        hp = _lib.LayerwiseHp(grad_scale=1.0 / world, clip_norm=self.clip_norm, lr=lr,
                              lr_t=lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if adaptive else lr,
                              momentum=self.opt.momentum, beta1=b1, beta2=b2, eps=self.opt.epsilon,
                              bias1=1.0 / (1.0 - b1 ** t) if adaptive else 1.0,
                              bias2=1.0 / (1.0 - b2 ** t) if adaptive else 1.0,
                              trust=self.opt.trust, ema_step=0.0 if ema_step is None else ema_step.value)
        descs, keep = self._param_descs()
        if getattr(self, '_ratios', None) is None or self._ratios.numel() != len(self.order):
            self._ratios = torch.ones(len(self.order), dtype=torch.float32, device=dev)
        sc = _scratch(st, 'opt_multi', L.y3_layerwise_update_multi_scratch_bytes(descs, len(self.order)), dev)
        _lib.check(L.y3_layerwise_update_multi(ctx, kind, descs, len(self.order), ctypes.byref(hp),
                                               None if ema_step is None else self._ema_arr, fw.ptr(self._ratios),
                                               fw.ptr(sc), ctypes.c_size_t(sc.numel())))

    def trust_ratios(self):
        """{op_name: the ratio the last apply_gradients used for that variable} (adamw: 1 everywhere; gamma, beta and
        biases: 1).  Synchronises the device once: meant for logging, not for every step."""
        if self.opt.kind not in Optimizer.LAYERWISE:
            raise RuntimeError("the '%s' rule has no trust ratios (adamw, lars and lamb report them)" % self.opt.kind)
        if getattr(self, '_ratios', None) is None:
            raise RuntimeError('trust_ratios() needs an apply_gradients() before it')
        values = self._ratios.cpu().tolist()
        return {v.op_name: values[i] for i, v in enumerate(self.order)}

    def step(self, images, y_true):
        """One training step on a batch; returns [total, xy, wh, conf, class] (device scalars):
        forward(is_training=True) -> compute_loss -> backward in ONE library call (y3_net_train_step), then the
        all-reduce join, L2, clip and update (y3_clip_update_multi)."""
        self._no_update_while_averaged('step()')
        x = fw.as_device_f32(images)
        self.model.img_size = [int(x.shape[1]), int(x.shape[2])]
        timing = None
        if self._calib is not None:
            k = self._calib['step']
            self.model.wgrad_stream = k < 4                   # steps 0-3 with the second stream, 4-6 without
            if k in (2, 3, 5, 6):
                timing = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                timing[0].record(torch.cuda.current_stream(x.device))
        else:
            self.model.wgrad_stream = self.wgrad_choice
        st, net, layer_vars = _prepare(self.model, x)
        n, h, w, _ = x.shape
        yt = [fw.as_device_f32(y) for y in y_true]
        for y, s in zip(yt, (32, 16, 8)):
            if tuple(y.shape) != (n, h // s, w // s, 3, 6 + int(self.model.class_num)):
                raise ValueError("y_true shape %s does not match the input size" % (tuple(y.shape),))
        arr = self._vars(layer_vars, x.device)
        opts, anc = _opts(self.model)
        loss5 = torch.empty(5, dtype=torch.float32, device=x.device)
        self.exchange.begin()
        if self.bn_sync is not None:
            self.bn_sync.begin()
        _checked(self.model, _lib.lib().y3_net_train_step(net, arr, fw.ptr(x), n, h, w, fw.ptr(yt[0]), fw.ptr(yt[1]), fw.ptr(yt[2]),
                                                          ctypes.byref(opts), fw.ptr(self.flat), fw.ptr(st['ws']),
                                                          ctypes.c_size_t(st['ws'].numel()), fw.ptr(loss5), self._ready_cb(), None))
        st.update(have_loss=True, fms=None, fm_ptrs=None)
        for wvar, bnv, bias in layer_vars:
            if bnv is not None:
                bnv[2].touch()
                bnv[3].touch()
        if self.capture is not None:
            self._fill_capture(st)
        self.apply_gradients()
        if self._calib is not None:
            c = self._calib
            if timing is not None:
                timing[1].record(torch.cuda.current_stream(x.device))
                timing[1].synchronize()
                (c['on'] if c['step'] < 4 else c['off']).append(timing[0].elapsed_time(timing[1]))
            c['step'] += 1
            if c['step'] == 7:
                self.wgrad_choice = min(c['on']) < 0.995 * min(c['off'])
                self.wgrad_calibration = dict(ms_with=min(c['on']), ms_without=min(c['off']))
                self._calib = None
        return [loss5[0], loss5[1], loss5[2], loss5[3], loss5[4]]
