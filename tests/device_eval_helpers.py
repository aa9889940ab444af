"""What the GPU tests of the device evaluators (test_voc_device_gpu.py, test_coco_device_gpu.py) build in common: batches in the
layout y3_nms leaves them in, and the synthetic set eval.py runs end to end on."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def nms_like(preds, image_ids, cap, dev):
    """The rows of `preds` that belong to `image_ids` in the layout y3_nms leaves detections in: (boxes [n,cap,4], scores [n,cap],
    labels [n,cap], counts [n]) device tensors; slots past an image's count hold poison.  Also returns the host concatenation of
    the live rows: image by image, an image's rows in the order of `preds`."""
    import torch
    n = len(image_ids)
    per_image = {k: [] for k in image_ids}
    for p in preds:
        if p[0] in per_image:
            per_image[p[0]].append(p)
    ob, osc = np.full((n, cap, 4), np.nan, np.float32), np.full((n, cap), np.nan, np.float32)
    ol, cnt, rows = np.full((n, cap), -5, np.int32), np.zeros(n, np.int32), []
    for i, img in enumerate(image_ids):
        for p in per_image[img]:
            ob[i, cnt[i]], osc[i, cnt[i]], ol[i, cnt[i]] = p[1:5], p[5], p[6]
            cnt[i] += 1
        rows += per_image[img]
    return tuple(torch.from_numpy(x).to(dev) for x in (ob, osc, ol, cnt)), rows


def eval_script_set(tmp_path):
    """A synthetic 6-image / 5-class set for eval.py with random weights, written under tmp_path.  Returns the arguments every
    run shares.  Resets the default graph (the caller takes the isolated_graph fixture)."""
    from PIL import Image
    import torch
    import yolov3_tensorflow_amd as y3
    from yolov3_tensorflow_amd.utils import misc_utils
    rng = np.random.RandomState(5)
    names = tmp_path / 'names.txt'
    names.write_text('\n'.join('c%d' % i for i in range(5)) + '\n')
    lines, obj = [], 0
    for i in range(6):
        w, h = int(rng.randint(120, 400)), int(rng.randint(120, 400))
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        path = tmp_path / ('im%d.png' % i)
        Image.fromarray(img).save(str(path))
        parts = ['%d' % i, str(path), '%d' % w, '%d' % h]
        for _ in range(int(rng.randint(2, 4))):
            x0, y0 = rng.uniform(0, w * 0.6), rng.uniform(0, h * 0.6)
            obj += 1
            parts += ['%d' % (obj % 5), '%.1f' % x0, '%.1f' % y0, '%.1f' % (x0 + rng.uniform(20, w * 0.35)),
                      '%.1f' % (y0 + rng.uniform(20, h * 0.35))]
        lines.append(' '.join(parts))
    ann = tmp_path / 'val.txt'
    ann.write_text('\n'.join(lines) + '\n')
    anchors = os.path.join(os.path.dirname(HERE), 'data', 'yolo_anchors.txt')
    y3.reset_default_graph()
    y3.set_init_seed(3)
    m = y3.yolov3(5, misc_utils.parse_anchors(anchors))
    with y3.variable_scope('yolov3'):
        m.forward(torch.zeros(1, 64, 64, 3))
    wfile = str(tmp_path / 'rand.weights')
    misc_utils.save_weights(y3.global_variables(scope='yolov3'), wfile)
    return ['--eval_file', str(ann), '--restore_path', wfile, '--anchor_path', anchors, '--class_name_path', str(names),
            '--img_size', '224', '160', '--letterbox_resize', 'true', '--batch_size', '4', '--score_threshold', '0.1',
            '--nms_topk', '20']
