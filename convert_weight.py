# coding: utf-8
"""Twin of the reference's convert_weight.py: darknet `.weights` -> a native checkpoint keyed by the TF variable
names (one `.npz`, see utils.misc_utils.Saver), which train.py / eval.py accept as --restore_path.

    python convert_weight.py [--weight_path ./data/darknet_weights/yolov3.weights] [--save_path .../yolov3.ckpt]
"""
from __future__ import division, print_function

import argparse


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--num_class', type=int, default=80)
    ap.add_argument('--weight_path', default='./data/darknet_weights/yolov3.weights')
    ap.add_argument('--save_path', default='./data/darknet_weights/yolov3.ckpt')
    ap.add_argument('--anchor_path', default='./data/yolo_anchors.txt')
    ap.add_argument('--spp', type=lambda text: str(text).lower() == 'true', default=False,
                    help='true: the YOLOv3-SPP architecture (yolov3-spp.weights, read in graph order like any darknet file)')
    a = ap.parse_args(argv)
    import torch
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd.utils.misc_utils import parse_anchors, load_weights, run_ops, Saver
    model = y3.yolov3(a.num_class, parse_anchors(a.anchor_path))
    model.spp = a.spp
    with y3.variable_scope('yolov3'):
        model.forward(torch.zeros((1, 64, 64, 3)))
    variables = y3.global_variables(scope='yolov3')
    run_ops(load_weights(variables, a.weight_path))
    path = Saver(variables).save(a.save_path)
    print('Native checkpoint has been saved to {}'.format(path))
    return path


if __name__ == '__main__':
    main()
