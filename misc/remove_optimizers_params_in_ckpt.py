# coding: utf-8
"""Strip the optimizer state from a native checkpoint (the reference's misc/remove_optimizers_params_in_ckpt.py for its TF
checkpoints): train.py's `.npz` files hold, next to every variable, its Momentum / Adam / RMSProp / AdamW / LARS / LAMB slots, `optimizer/step` and
`global_step` (utils.misc_utils.Saver) - two to three times the size the forward needs.  A run with --ema_decay also stores
every trained variable's moving average as '<variable>/ExponentialMovingAverage'; those keys are dropped as well, and with
--use_ema true the averages are what the stripped file holds under the variables' own names.

    python misc/remove_optimizers_params_in_ckpt.py checkpoint/best_model.npz [--output shrinked_ckpt/shrinked.npz]
                                                    [--use_ema true]
"""
import argparse
import os
import sys

import numpy as np

SLOT_SUFFIXES = ('/Momentum', '/Adam', '/Adam_1', '/RMSProp', '/RMSProp_1',
                 '/AdamW', '/AdamW_1', '/LARS', '/LAMB', '/LAMB_1')
EMA_SUFFIX = '/ExponentialMovingAverage'
BOOKKEEPING = ('optimizer/step', 'global_step')


def shrink(src, dst, use_ema=False):
    """Copies the variables of checkpoint `src` to `dst`; returns (kept keys, dropped keys).  use_ema: a variable whose moving
    average the file holds (in the variable's shape) is written with that average as its value."""
    ckpt = np.load(src if src.endswith('.npz') else src + '.npz')
    drop = [k for k in ckpt.files if k in BOOKKEEPING or k.endswith(SLOT_SUFFIXES) or k.endswith(EMA_SUFFIX)]
    keep = [k for k in ckpt.files if k not in drop]
    out = {k: ckpt[k] for k in keep}
    if use_ema:
        for k in keep:
            if k + EMA_SUFFIX in ckpt.files and ckpt[k + EMA_SUFFIX].shape == ckpt[k].shape:
                out[k] = ckpt[k + EMA_SUFFIX]
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst if dst.endswith('.npz') else dst + '.npz', 'wb') as f:
        np.savez(f, **out)
    return keep, drop


def main(argv=None):
    ap = argparse.ArgumentParser(description="drop the optimizer slots from a native .npz checkpoint")
    ap.add_argument('ckpt_path')
    ap.add_argument('--output', default=os.path.join('shrinked_ckpt', 'shrinked.npz'))
    ap.add_argument('--use_ema', type=lambda text: str(text).lower() == 'true', default=False,
                    help='true: write the weight moving averages under the variables\' own names')
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    keep, drop = shrink(args.ckpt_path, args.output, use_ema=args.use_ema)
    print('%s: kept %d arrays, dropped %d optimizer / moving-average arrays' % (args.output, len(keep), len(drop)))
    return keep, drop


if __name__ == '__main__':
    main()
