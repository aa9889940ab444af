"""Run test_single_image.py or video_test.py on the YOLOv3-SPP architecture.

    python tools/run_spp.py test_single_image.py ./data/demo_data/messi.jpg --restore_path ./data/darknet_weights/yolov3-spp.weights
    python tools/run_spp.py video_test.py ./data/demo_data/video.avi --restore_path spp_checkpoint.npz

The two inference scripts build their model themselves and have no --spp option (train.py, eval.py and convert_weight.py
do).  This sets what a new model's `spp` starts as (yolov3.default_spp) and then runs the named script's main() with the rest
of the command line, unchanged.  Returns what that main() returns."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ('test_single_image', 'video_test')


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    name = os.path.splitext(os.path.basename(argv[0]))[0] if argv else ''
    if name not in SCRIPTS:
        raise SystemExit('usage: python tools/run_spp.py {%s}.py <the script\'s own arguments>' % '|'.join(SCRIPTS))
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from yolov3_tensorflow_amd.model import yolov3
    before = yolov3.default_spp
    yolov3.default_spp = True
    try:
        return importlib.import_module(name).main(argv[1:])
    finally:
        yolov3.default_spp = before


if __name__ == '__main__':
    main()
