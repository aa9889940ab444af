# coding: utf-8
"""Mirror of the reference's utils/misc_utils.py for the pieces on the hot path:
load_weights (darknet .weights loader), parse_anchors, read_class_names, AverageMeter,
config_learning_rate, config_optimizer.  save_weights (the inverse of load_weights) is an addition used
to produce synthetic checkpoints in the exact darknet format.
"""
from __future__ import division, print_function

import math

import numpy as np


def make_summary(name, val):
    """reference utils/misc_utils.py:10-11 builds a TensorBoard Summary proto; without TensorFlow the (tag, value) pair is
    what there is to record (the compat layer's FileWriter keeps them, train.py of this package logs them)."""
    return (name, float(val))


def shuffle_and_overwrite(file_name):
    """reference utils/misc_utils.py:48-53."""
    import random
    content = open(file_name, 'r').readlines()
    random.shuffle(content)
    with open(file_name, 'w') as f:
        for line in content:
            f.write(line)


def update_dict(ori_dict, new_dict):
    """reference utils/misc_utils.py:56-61."""
    if not ori_dict:
        return new_dict
    for key in ori_dict:
        ori_dict[key] += new_dict[key]
    return ori_dict


class AverageMeter(object):
    """Running mean with the attribute names the training/eval loops read (utils/misc_utils.py:14-28)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val, self.average, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.average = self.sum / float(self.count)


def parse_anchors(anchor_path):
    """Comma-separated anchor file -> float32 [N, 2] of (w, h) pairs (utils/misc_utils.py:31-37)."""
    with open(anchor_path, 'r') as f:
        flat = np.asarray(f.read().split(','), np.float32)
    return flat.reshape(-1, 2)


def read_class_names(class_name_path):
    """One class name per line -> {id: name} (utils/misc_utils.py:40-45)."""
    with open(class_name_path, 'r') as f:
        return {i: line.strip('\n') for i, line in enumerate(f)}


class AssignOp(object):
    """What load_weights returns in place of tf.assign ops: run() copies the array into the variable
    with shape validation (tf.assign(validate_shape=True), utils/misc_utils.py:99,110,123)."""

    def __init__(self, var, value):
        self.var, self.value = var, value

    def run(self):
        self.var.assign(self.value, validate_shape=True)
        return self.var

    __call__ = run


def run_ops(ops):
    """sess.run(load_ops) equivalent (convert_weight.py:31)."""
    for op in ops:
        op.run()


def _layer_key(var):
    # the loader keys on the second-to-last path component of the variable name (utils/misc_utils.py:88-102)
    return var.name.split('/')[-2]


def _conv_groups(var_list):
    """Walk a creation-ordered variable list the way the reference loader does and yield, per conv layer,
    (kernel_var, (gamma, beta, mean, var) or None, bias_var or None).  The walk stops one short of the end
    like the reference (`while i < len(var_list) - 1`), so a trailing lone variable is ignored."""
    i, n = 0, len(var_list)
    while i < n - 1:
        head, nxt = var_list[i], var_list[i + 1]
        if 'Conv' not in _layer_key(head):
            i += 1   # (the reference would spin forever here; such lists never occur)
            continue
        if 'BatchNorm' in _layer_key(nxt):
            yield head, tuple(var_list[i + 1:i + 5]), None
            i += 5
        elif 'Conv' in _layer_key(nxt):
            yield head, None, nxt
            i += 2
        else:
            yield head, None, None
            i += 1


def load_weights(var_list, weights_file):
    """Darknet .weights -> assign ops for `var_list` (reference utils/misc_utils.py:70-126).

    var_list: network variables in creation order (e.g. global_variables(scope='yolov3')).
    File: 5 x int32 header (ignored), then a float32 stream; per conv layer
      BN'd : beta, gamma, moving_mean, moving_variance (FILE order; the variable order is gamma first)
      else : bias
      then the kernel as (Cout, Cin, kh, kw), transposed here to HWIO.
    Returns a list of AssignOp; execute with run_ops(ops).

    The stream is read with the FILE's layer sizes, not blindly with the model's: a darknet file does not name its
    class count, but the stream length does (the only layers whose size depends on it are the bias'd detection convs,
    Cout = 3*(5+C)).  When the length does not fit the model's class count but fits another one, the detection layers
    are cut with the file's Cout so that every later layer is read from the right offset; their AssignOps then carry
    file-shaped arrays and raise ValueError when run (tf.assign(validate_shape=True)) — unless the caller drops them,
    which is exactly what train.py's default restore_exclude does when fine-tuning a COCO file on another class count.
    (The reference restores by NAME from a converted TF checkpoint, so its exclude works the same way.)  A length that
    fits no class count raises ValueError (a truncated / over-long file, or not a darknet file at all).
    """
    with open(weights_file, "rb") as fp:
        np.fromfile(fp, dtype=np.int32, count=5)
        stream = np.fromfile(fp, dtype=np.float32)

    groups = list(_conv_groups(var_list))

    def layer_count(kernel, bn, bias, det_cout=None):
        kh, kw, cin, cout = kernel.shape.as_list()
        if det_cout is not None and bn is None and bias is not None:
            cout = det_cout
        return kh * kw * cin * cout + (4 * cout if bn is not None else cout if bias is not None else 0)

    expected = sum(layer_count(*g) for g in groups)
    det_cout = None
    if expected != stream.size:
        dets = [g for g in groups if g[1] is None and g[2] is not None]
        couts = set(g[0].shape.as_list()[3] for g in dets)
        per_cout = sum(g[0].shape.as_list()[0] * g[0].shape.as_list()[1] * g[0].shape.as_list()[2] + 1 for g in dets)
        rest = expected - (per_cout * couts.pop() if len(couts) == 1 else 0)
        cand = (stream.size - rest) // per_cout if (dets and not couts and per_cout) else 0
        if not dets or couts or cand <= 0 or rest + per_cout * cand != stream.size or cand % 3 or cand // 3 <= 5:
            raise ValueError("%s holds %d float32 values, the variables need %d: truncated / over-long file, or not a "
                             "darknet file of this architecture" % (weights_file, stream.size, expected))
        det_cout = int(cand)        # the file was written for (det_cout / 3 - 5) classes

    pos = [0]

    def take(shape):
        count = int(np.prod(shape))
        chunk = stream[pos[0]:pos[0] + count]
        pos[0] += count
        return chunk

    ops = []
    for kernel, bn, bias in _conv_groups(var_list):
        if bn is not None:
            gamma, beta, mean, variance = bn
            for v in (beta, gamma, mean, variance):
                ops.append(AssignOp(v, take(v.shape.as_list()).reshape(v.shape.as_list())))
        elif bias is not None:
            bshape = bias.shape.as_list() if det_cout is None else [det_cout]
            ops.append(AssignOp(bias, take(bshape).reshape(bshape)))
        kh, kw, cin, cout = kernel.shape.as_list()
        if det_cout is not None and bn is None and bias is not None:
            cout = det_cout
        oihw = take((cout, cin, kh, kw)).reshape(cout, cin, kh, kw)
        ops.append(AssignOp(kernel, np.transpose(oihw, (2, 3, 1, 0))))
    return ops


def save_weights(var_list, weights_file, header=(0, 2, 0, 0, 0)):
    """Inverse of load_weights: write the variables as a darknet .weights file (same traversal)."""
    chunks = []
    for kernel, bn, bias in _conv_groups(var_list):
        if bn is not None:
            gamma, beta, mean, variance = bn
            chunks.extend(v.numpy().astype(np.float32).ravel() for v in (beta, gamma, mean, variance))
        elif bias is not None:
            chunks.append(bias.numpy().astype(np.float32).ravel())
        hwio = kernel.numpy().astype(np.float32)
        chunks.append(np.ascontiguousarray(np.transpose(hwio, (3, 2, 0, 1))).ravel())
    with open(weights_file, "wb") as fp:
        np.asarray(header, np.int32).tofile(fp)
        np.concatenate(chunks).astype(np.float32).tofile(fp)


# ------------------------------------------------------------------------------------------------------------
# native checkpoints keyed by the TF variable names (stands in for tf.train.Saver in
# train.py:81-82,101-124,169-171,213-216 and convert_weight.py)
# ------------------------------------------------------------------------------------------------------------
def _in_scopes(name, scopes):
    return any(name == s or name.startswith(s + '/') for s in scopes)


def get_variables_to_restore(variables, include=None, exclude=None):
    """tf.contrib.framework.get_variables_to_restore(include, exclude) over an explicit variable list: scopes match
    whole name components ('yolov3/yolov3_head/Conv_6' does not match '.../Conv_60')."""
    keep = list(variables) if include is None else [v for v in variables if _in_scopes(v.op_name, include)]
    return keep if exclude is None else [v for v in keep if not _in_scopes(v.op_name, exclude)]


# slot names TF1 gives the optimizer variables (utils/misc_utils.py:151-161 optimizers)
_SLOT_NAMES = {'momentum': ('Momentum',), 'adam': ('Adam', 'Adam_1'), 'rmsprop': ('RMSProp', 'RMSProp_1'),
               'sgd': (),
               # the layer-wise rules (not TF1's: named in its pattern)
               'adamw': ('AdamW', 'AdamW_1'), 'lars': ('LARS',), 'lamb': ('LAMB', 'LAMB_1')}
# the name TF1 gives a variable's moving average (tf.train.ExponentialMovingAverage.average_name)
EMA_SUFFIX = '/ExponentialMovingAverage'


def has_averages(save_path):
    """True when the native checkpoint at save_path stores weight moving averages."""
    return any(k.endswith(EMA_SUFFIX) for k in np.load(Saver._path(save_path)).files)


class Saver(object):
    """A checkpoint is one `.npz` file whose keys are the variables' TF names ('yolov3/darknet53_body/Conv/weights',
    ...); with an optimizer, its slot variables are stored as '<variable>/<SlotName>' with TF1's slot names and
    `global_step` as a scalar.  restore() assigns every variable of `var_list` and raises KeyError, like TF's
    "Key ... not found in checkpoint", when one is missing; arrays are shape-checked by Variable.assign."""

    def __init__(self, var_list):
        self.var_list = list(var_list)

    @staticmethod
    def _path(path):
        return path if path.endswith('.npz') else path + '.npz'

    def save(self, save_path, optimizer=None, global_step=None, averages=None):
        """averages: a training.Trainer that keeps a weight moving average.  Every average is stored as
        '<variable>/ExponentialMovingAverage' (TF1's shadow name).  The variable's own key always holds the RAW iterate, also
        when the call is made inside trainer.averaged(), so a run resumed from the file continues both."""
        out = {v.op_name: v.numpy() for v in self.var_list}
        if averages is not None:
            names = set(out)
            for name, t in averages.raw_tensors().items():
                if name in names:
                    out[name] = t.detach().cpu().numpy()
            for name, t in averages.ema_tensors().items():
                if name in names:
                    out[name + EMA_SUFFIX] = t.detach().cpu().numpy()
        if optimizer is not None:
            for name, slots in optimizer.slots.items():
                for slot_name, t in zip(_SLOT_NAMES[optimizer.kind], slots):
                    if t is not None:
                        out[name + '/' + slot_name] = t.detach().cpu().numpy()
            out['optimizer/step'] = np.int64(optimizer.step)
        if global_step is not None:
            out['global_step'] = np.float64(global_step)
        path = self._path(save_path)
        with open(path, 'wb') as f:
            np.savez(f, **out)
        return path

    def restore(self, save_path, optimizer=None, variables=True, averages=None, use_ema=False):
        """Returns the stored global_step (or None).  variables=False leaves the variables alone and loads only the
        optimizer slots (of the variables in var_list whose stored slots match the variable's shape) and its step —
        what resuming needs AFTER a filtered variable restore (train.py: restore_exclude must stay excluded).
        averages: a training.Trainer that keeps a weight moving average; the stored averages of the variables in var_list
        that are present and match in shape become its shadows, the others keep their start value.
        use_ema=True assigns the stored AVERAGE to the variable itself where the file holds one of the variable's shape
        (TF's variables_to_restore() idiom for evaluation); a variable without one takes its own key."""
        import torch
        ckpt = np.load(self._path(save_path))
        if variables:
            for v in self.var_list:
                if v.op_name not in ckpt.files:
                    raise KeyError('Key %s not found in checkpoint %s' % (v.op_name, save_path))
                key = v.op_name
                if use_ema and key + EMA_SUFFIX in ckpt.files and tuple(ckpt[key + EMA_SUFFIX].shape) == tuple(v.shape):
                    key += EMA_SUFFIX
                v.assign(ckpt[key], validate_shape=True)
        if averages is not None:
            for v in self.var_list:
                key = v.op_name + EMA_SUFFIX
                if key in ckpt.files and tuple(ckpt[key].shape) == tuple(v.shape):
                    averages.ema_assign(v.op_name, ckpt[key])
        if optimizer is not None:
            for v in self.var_list:
                keys = [v.op_name + '/' + s for s in _SLOT_NAMES[optimizer.kind]]
                if keys and all(k in ckpt.files and tuple(ckpt[k].shape) == tuple(v.shape) for k in keys):
                    slots = [torch.as_tensor(ckpt[k]).to(v.tensor.device) for k in keys]
                    optimizer.slots[v.op_name] = tuple(slots + [None] * (2 - len(slots)))
            if 'optimizer/step' in ckpt.files:
                optimizer.step = int(ckpt['optimizer/step'])
        return float(ckpt['global_step']) if 'global_step' in ckpt.files else None


def restore_for_inference(variables, save_path, use_ema=False):
    """What an inference script (eval.py --use_ema) does with a native .npz: Saver.restore, with the stored weight moving
    averages in place of the raw weights when use_ema is set.  A file without averages is said so, and read as it is."""
    if use_ema and not has_averages(save_path):
        print('--use_ema true: %s holds no weight moving averages (it was not written by a run with --ema_decay); '
              'using the raw weights' % save_path)
        use_ema = False
    return Saver(variables).restore(save_path, use_ema=use_ema)


def config_learning_rate(args, global_step):
    """reference utils/misc_utils.py:129-148, evaluated eagerly: returns the python float learning rate
    for `global_step` (float).  Raises ValueError for an unknown lr_type like the reference."""
    if args.lr_type == 'exponential':
        # tf.train.exponential_decay(staircase=True) then max with the lower bound
        lr_tmp = args.learning_rate_init * args.lr_decay_factor ** math.floor(global_step / args.lr_decay_freq)
        return max(lr_tmp, args.lr_lower_bound)
    elif args.lr_type == 'cosine_decay':
        train_steps = (args.total_epoches - float(args.use_warm_up) * args.warm_up_epoch) * args.train_batch_num
        return args.lr_lower_bound + 0.5 * (args.learning_rate_init - args.lr_lower_bound) * \
            (1 + math.cos(global_step / train_steps * np.pi))
    elif args.lr_type == 'cosine_decay_restart':
        # tf.train.cosine_decay_restarts(lr, step, first_decay_steps, t_mul=2.0, m_mul=1.0, alpha=0)
        first, t_mul = float(args.lr_decay_freq), 2.0
        completed = global_step / first
        i_restart = math.floor(math.log(1.0 - completed * (1.0 - t_mul)) / math.log(t_mul))
        sum_r = (1.0 - t_mul ** i_restart) / (1.0 - t_mul)
        completed_fraction = (completed - sum_r) / t_mul ** i_restart
        return args.learning_rate_init * 0.5 * (1.0 + math.cos(math.pi * completed_fraction))
    elif args.lr_type == 'fixed':
        return float(args.learning_rate_init)
    elif args.lr_type == 'piecewise':
        # tf.train.piecewise_constant: values[i] for boundaries[i-1] < step <= boundaries[i]
        for b, v in zip(args.pw_boundaries, args.pw_values):
            if global_step <= b:
                return float(v)
        return float(args.pw_values[-1])
    else:
        raise ValueError('Unsupported learning rate type!')


def config_optimizer(optimizer_name, learning_rate, decay=0.9, momentum=0.9, trust=0.001):
    """reference utils/misc_utils.py:151-161: returns an optimizer object for the train step
    (yolov3_tensorflow_amd.training).  Beyond the reference's four names: 'adamw', 'lars' (momentum and the trust
    coefficient `trust`) and 'lamb', the layer-wise rules for large global batches."""
    from .. import training
    if optimizer_name in ('adamw', 'lamb'):
        return training.Optimizer(optimizer_name, learning_rate)
    elif optimizer_name == 'lars':
        return training.Optimizer('lars', learning_rate, momentum=momentum, trust=trust)
    elif optimizer_name == 'momentum':
        return training.Optimizer('momentum', learning_rate, momentum=momentum)
    elif optimizer_name == 'rmsprop':
        return training.Optimizer('rmsprop', learning_rate, decay=decay, momentum=momentum)
    elif optimizer_name == 'adam':
        return training.Optimizer('adam', learning_rate)
    elif optimizer_name == 'sgd':
        return training.Optimizer('sgd', learning_rate)
    else:
        raise ValueError('Unsupported optimizer type!')
