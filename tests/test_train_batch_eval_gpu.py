"""train.py --batch_eval_on_device true prints the same "Last batch: rec / prec" values as without the flag on the same seed:
the toy set of tests/test_train_script_gpu.py (8 images of 160x160, 3 classes, one batch per epoch), six steps from random
initialisation, the training batch evaluated every second step."""
import os
import sys

import pytest

from test_train_script_gpu import make_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_batch_line_is_the_same_with_the_flag(tmp_path, capsys, isolated_graph):
    import yolov3_tensorflow_amd as y3
    sys.path.insert(0, ROOT)
    import train as train_script
    ann, names = make_dataset(tmp_path)
    lines, recalls = {}, {}
    for flag in ('false', 'true'):
        y3.reset_default_graph()
        hist = train_script.main([
            '--train_file', ann, '--val_file', ann, '--restore_path', '', '--save_dir', str(tmp_path / ('ckpt_' + flag)),
            '--progress_log_path', '', '--anchor_path', os.path.join(ROOT, 'data', 'yolo_anchors.txt'),
            '--class_name_path', names, '--batch_size', '8', '--img_size', '160', '160', '--letterbox_resize', 'false',
            '--total_epoches', '6', '--train_evaluation_step', '2', '--val_evaluation_epoch', '1000', '--save_epoch', '1000',
            '--batch_norm_decay', '0.9', '--optimizer_name', 'adam', '--learning_rate_init', '1e-3', '--lr_type', 'fixed',
            '--update_part', 'None', '--multi_scale_train', 'false', '--use_warm_up', 'false', '--warm_up_epoch', '0',
            '--use_label_smooth', 'false', '--use_focal_loss', 'false', '--weight_decay', '0', '--augment', 'false',
            '--num_threads', '4', '--seed', '0', '--batch_eval_on_device', flag])
        lines[flag] = [l for l in capsys.readouterr().out.splitlines() if 'Last batch: rec:' in l]
        recalls[flag] = hist['recall']
    print('\n'.join(lines['true']))
    assert len(lines['false']) == 3 and lines['true'] == lines['false']
    assert recalls['true'] == recalls['false'] and len(recalls['true']) == 3
