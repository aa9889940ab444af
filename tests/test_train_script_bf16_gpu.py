"""test_train_script_gpu.py's 201-epoch memorisation run through the real train.py loop, with the mixed-precision train step
(`--compute_dtype bf16`): same synthetic set, same options, same gates - the loss falls below half, and the training-batch
recall and the mAP (inference in the same mode) exceed 0.8."""
import os
import sys

import numpy as np
import pytest

from test_train_script_gpu import ROOT, make_dataset

pytestmark = pytest.mark.gpu


def test_bf16_training_loop_memorises_the_set(tmp_path, capsys, isolated_graph):
    import yolov3_tensorflow_amd as y3
    sys.path.insert(0, ROOT)
    import train as train_script
    ann, names = make_dataset(tmp_path)
    y3.reset_default_graph()
    hist = train_script.main([
        '--train_file', ann, '--val_file', ann, '--restore_path', '', '--save_dir', str(tmp_path / 'ckpt'),
        '--progress_log_path', str(tmp_path / 'progress.log'), '--anchor_path', os.path.join(ROOT, 'data', 'yolo_anchors.txt'),
        '--class_name_path', names, '--batch_size', '8', '--img_size', '160', '160', '--letterbox_resize', 'false',
        '--total_epoches', '201', '--train_evaluation_step', '50', '--val_evaluation_epoch', '200', '--batch_norm_decay', '0.9', '--save_epoch', '1000',
        '--optimizer_name', 'adam', '--learning_rate_init', '1e-3', '--lr_type', 'piecewise', '--pw_boundaries', '140',
        '--pw_values', '1e-3', '1e-4', '--update_part', 'None',
        '--multi_scale_train', 'false', '--use_warm_up', 'false', '--warm_up_epoch', '0', '--use_label_smooth', 'false',
        '--use_focal_loss', 'false', '--score_threshold', '0.3', '--nms_topk', '20', '--weight_decay', '0', '--augment', 'false',
        '--num_threads', '4', '--compute_dtype', 'bf16'])
    out = capsys.readouterr().out
    loss = np.array(hist['loss'])
    print('bf16: loss first %.2f, min %.2f, last %.2f; recalls %s; mAP %s' % (loss[0], loss.min(), loss[-1], hist['recall'],
                                                                             hist['mAP']))
    assert np.isfinite(loss).all()
    assert loss[-10:].mean() < 0.5 * loss[:3].mean()
    assert 'Last batch: rec:' in out and 'EVAL: Recall:' in out
    assert hist['recall'][-1] > 0.8 and hist['mAP'][-1] > 0.8
