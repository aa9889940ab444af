#!/usr/bin/env python
"""Two warm-up train steps and one more, at batch 2 on a small non-square input, for a kernel trace of the train step:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/train_step_once.py f32_wino|bf16
    python tools/launch_sequence.py DIR/*/t_kernel_trace.csv

Weight gradients on the second stream; synthetic variables and targets (every step launches the same kernels)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))

N, H, W, CLASS_NUM = 2, 96, 160, 20


def main():
    import torch
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd import training
    from yolov3_tensorflow_amd.utils.misc_utils import config_optimizer
    from oracle import yolo_ref
    from conftest import COCO_ANCHORS
    from test_train_gpu import _blob_images_hw
    from test_train_sizes_gpu import _targets
    model = y3.yolov3(CLASS_NUM, COCO_ANCHORS)
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros(1, 32, 32, 3))
    params = yolo_ref.synthetic_params(CLASS_NUM, seed=1)
    for v in y3.global_variables(scope='yolov3'):
        v.assign(params[v.op_name])
    model.compute_dtype = sys.argv[1]
    trainer = training.Trainer(model, config_optimizer('sgd', 1e-3), wgrad_stream=True)
    x, yts = _blob_images_hw(3, N, H, W), _targets(4, N, H, W)
    with y3.variable_scope('yolov3'):
        for _ in range(3):
            loss = trainer.step(x, yts)
    torch.cuda.synchronize()
    print('%s %dx%dx%d: loss %r' % (sys.argv[1], N, H, W, float(loss[0])))


if __name__ == '__main__':
    main()
