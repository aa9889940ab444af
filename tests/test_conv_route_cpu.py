"""The conv route table (which kernel form every layer takes per net dtype and input shape, and the workspaces sized for it)
against tests/golden/conv_routes.json, recorded from the library before the route of each layer was decided in one place
(csrc/y3_abi.hip y3_route_*).  Host-only ABI calls on a net created without a context (tests/golden/make_route_golden.py).
One column was re-recorded since: 'streamk' (y3_net_layer_is_streamk).  y3_conv_schedule_impl used to read uninitialised
fields and answered 0 for every layer; it now gives the schedule y3_launch_conv picks.  One column was added:
'train_workspace_sel', the train step's workspace for every dtype (bf16 included), the all-trainable table and every partial
update_vars of tests/test_train_gpu.py, stream off and on - recorded from the library before the train step's host code
(csrc/y3_net_train.hip) was split into named steps, which must reproduce every number.

Some entries depend on the device the library sees (the fused stem / residual block need the device to offer their kernels'
LDS): the file holds one table made without a device and one made on an MI355X."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_route_golden  # noqa: E402


@pytest.fixture(scope='module')
def tables():
    from yolov3_tensorflow_amd import build
    build.build(verbose=False)
    import torch
    with open(make_route_golden.OUT) as f:
        want = json.load(f)['device' if torch.cuda.is_available() else 'host']
    return want, make_route_golden.table()


def test_route_table_covers_every_net_dtype_and_shape(tables):
    want, got = tables
    assert sorted(got) == sorted(want)
    for n, h, w in ((32, 416, 416), (16, 608, 608), (64, 416, 416), (4, 256, 256), (3, 320, 320), (2, 416, 608)):
        for dt in ('dtype0', 'dtype1', 'dtype2', 'dtype3', 'dtype4+alt'):
            assert '%s/%dx%dx%d' % (dt, n, h, w) in want


@pytest.mark.parametrize('field', ['fused', 'streamk', 'bf16_tile', 'workspace', 'train_workspace', 'train_workspace_sel'])
def test_route_table_matches_golden(tables, field):
    want, got = tables
    bad = [k for k in sorted(want) if want[k].get(field) != got[k].get(field)]
    assert not bad, '%s differs at %s: want %s, got %s' % (field, bad[0], want[bad[0]].get(field), got[bad[0]].get(field))
