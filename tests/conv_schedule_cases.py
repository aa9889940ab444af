"""The shapes of tests/test_conv_schedules_gpu.py and the schedule each one exists to reach.  tests/test_conv_schedules_cpu.py
pins the schedules against the library's host rules (y3_conv_schedule, the weight gradient's split count) without a device;
the GPU tests assert them again ahead of every launch.

Schedules (y3_conv_schedule): 0 = one workgroup per tile, 1 = stream-K, 2 = the resident walk of the 64x64 tiles."""
import ctypes

ONE_PER_TILE, STREAMK, RESIDENT = 0, 1, 2


def desc(n, h, w, cin, c_up, cout, k, stride, act=0):
    from yolov3_tensorflow_amd import _lib
    return _lib.ConvDesc(n, h, w, cin, c_up, cout, k, stride, act)


def schedule(L, n, h, w, cin, c_up, cout, k, stride, taps=0, workspace=1):
    return L.y3_conv_schedule(ctypes.byref(desc(n, h, w, cin, c_up, cout, k, stride)), taps, workspace)


# ---- 1. weight gradient: (n, h, w, k, stride, cin, cout, dz_stride, K-steps of a ragged last split or None) ----------------
# splits x K-steps per split as the split rule gave them when the cases were chosen (the tests read the real count):
WGRAD = [
    (3, 150, 146, 1, 1, 64, 32, 32, 4),        # 411 x 5, last split 4; M % 32 = 4; the 32-wide tile
    (4, 94, 100, 3, 2, 32, 64, 64, None),      # 147 x 2; stride 2, the 64-wide tile
    (8, 26, 26, 1, 1, 256, 255, 256, 1),       # 57 x 3, last split 1; detection width, dz row stride 256
    (3, 37, 37, 3, 1, 64, 128, 128, None),     # 43 x 3; M % 32 = 11; Winograd-eligible
    (2, 90, 92, 3, 2, 128, 256, 256, None),    # 26 x 5; stride 2, the 128-wide tile
    (3, 61, 67, 1, 1, 128, 64, 64, None),      # 192 x 2; M % 32 = 5
    (3, 52, 50, 1, 1, 256, 75, 96, None),      # 122 x 2; the 20-class detection conv, M % 32 = 24
    (7, 26, 26, 1, 1, 512, 18, 32, None),      # 74 x 2; the one-class detection conv, M % 32 = 28
]
WGRAD_SPLITS = [(411, 5), (147, 2), (57, 3), (43, 3), (26, 5), (192, 2), (122, 2), (74, 2)]


def wgrad_split(L, n, h, w, k, stride, cin, cout):
    """(splits, K-steps per split, K-steps of the last split, M % 32) from the library's scratch size."""
    d = desc(n, h, w, cin, 0, cout, k, stride)
    ns = (L.y3_conv_wgrad_scratch_bytes(ctypes.byref(d)) - 256) // (k * k * cin * cout * 4)
    m = n * (h // stride) * (w // stride)
    ksteps = -(-m // 32)
    chunk = -(-ksteps // ns)
    return ns, chunk, ksteps - (ns - 1) * chunk, m % 32


# ---- 2. data gradient on stream-K: the FORWARD layer (n, h, w, cin, cout); the gradient conv is cout -> cin -------------------
# stream-K asks Cout' = fwd cin >= 128, >= 32 tiles and (tiles / 8) * taps * cout / 32 >= 64
DGRAD_S1 = [
    (3, 37, 37, 128, 64),      # gradient conv 64 -> 128: 33 tiles, ragged M, odd map
    (3, 37, 37, 256, 64),      # gradient conv 64 -> 256: 66 tiles
]
# stride 2, fwd 128 -> 256 at h x w = 90 x 92: parity classes of 1, 2, 2, 4 taps over n x 45 x 46 rows
DGRAD_S2 = [
    (2, 90, 92, 128, 256, (ONE_PER_TILE, STREAMK, STREAMK, STREAMK)),    # 33 tiles: the one-tap class stays data-parallel
    (4, 90, 92, 128, 256, (STREAMK, STREAMK, STREAMK, STREAMK)),         # 65 tiles
]
PARITY_TAPS = (1, 2, 2, 4)

# ---- 3. the resident walk, forward: (name, n, h, w, cin, c_up, cout, act, schedule) ------------------------------------------
FWD = [
    ('1040 tiles', 3, 27, 51, 32, 0, 1024, 1, RESIDENT),           # 65 x 16
    ('1024 tiles', 1, 64, 64, 32, 0, 1024, 1, ONE_PER_TILE),       # the neighbour below the threshold
    ('8176 tiles', 1, 511, 64, 32, 0, 1024, 1, RESIDENT),          # eight tiles per workgroup, the last run shorter
    ('8192 tiles', 1, 512, 64, 32, 0, 1024, 1, ONE_PER_TILE),      # the neighbour above the range
    ('odd cout', 4, 64, 65, 32, 0, 255, 0, RESIDENT),              # 260 x 4; the per-element epilogue, linear, a shift
    ('upsample+concat', 2, 128, 130, 64, 32, 128, 1, RESIDENT),    # 520 x 2; 32 upsampled + 32 route channels
]
FWD_STATS = (2, 128, 130, 32, 128)                                 # 520 x 2 tiles, RESIDENT, with the BN statistics

# ---- 4. the fused BN backward reduction: the FORWARD 1x1 layer (n, h, w, cin, cout, dz_stride, tile rows, schedule) ----------
DGRAD_BN = [
    (3, 20, 28, 32, 64, 64, 128, ONE_PER_TILE),      # 128x32 tile, ragged M (1680 = 13 x 128 + 16)
    (3, 20, 28, 64, 128, 128, 128, ONE_PER_TILE),    # 128x64 tile: eight passes, residual and z reloaded mid-tile
    (3, 20, 28, 128, 64, 64, 64, ONE_PER_TILE),      # 64x64 tile
    (2, 128, 65, 256, 128, 128, 64, RESIDENT),       # 260 x 4 tiles on the resident walk
    (3, 20, 28, 128, 255, 256, 64, ONE_PER_TILE),    # a detection conv reading a BN layer: dz row stride 256
]


# ---- 5. the host answers every launcher, planner and buffer size depends on --------------------------------------------------
# (query, (n, h, w, cin, c_up, cout, k, stride), further arguments, y3_debug_conv_range_limit in force or 0, answer).  The
# answers were recorded from the library as it stood BEFORE the conv launchers were moved onto one host path and one tile table
# per kernel family; they are not derived from that code.  Every branch of every ladder: the statistics rows of the fp32 forward
# (k = 1 and 3, Cout 32 / 64 / 128, stride 1 and 2, a ragged last block: 3 x 20 x 28 = 13 x 128 + 16 rows), the fused BN-backward
# rows (Cin 64 and 128), the Winograd counts on an odd map, the bf16 training rows at M = 128 and 129, the schedule of each
# shape with and without a workspace, the four parity classes of a stride-2 data gradient (y3_conv_schedule's conv is the one
# launched: [n, h/2, w/2, fwd cout] -> fwd cin), the workspace size, and four launches cut in two by a lowered range limit.
HOST_ANSWERS = [
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 32, 1, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 1, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 1, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 32, 1, 2), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 32, 1, 2), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 1, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 1, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 64, 1, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 1, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 1, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 64, 1, 2), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 64, 1, 2), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 1, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 1, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 128, 1, 1), (0,), 0, 27),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 128, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 1, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 1, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 128, 1, 2), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 128, 1, 2), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 1, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 1, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 32, 3, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 32, 3, 2), (0,), 0, 4),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 32, 3, 2), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 3, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 32, 3, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 64, 3, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 64, 3, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 64, 3, 2), (0,), 0, 4),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 64, 3, 2), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 3, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 64, 3, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 128, 3, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 128, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 64, 0, 128, 3, 2), (0,), 0, 4),
    ('y3_conv_workspace_bytes', (3, 20, 28, 64, 0, 128, 3, 2), (), 0, 33556480),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 3, 2), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 64, 0, 128, 3, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 128, 0, 64, 1, 1), (0,), 0, 14),
    ('y3_conv_workspace_bytes', (3, 20, 28, 128, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 128, 0, 64, 1, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 128, 0, 64, 1, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 20, 28, 128, 0, 128, 1, 1), (0,), 0, 27),
    ('y3_conv_workspace_bytes', (3, 20, 28, 128, 0, 128, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 128, 0, 128, 1, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 20, 28, 128, 0, 128, 1, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 13, 13, 64, 0, 128, 3, 1), (0,), 0, 4),
    ('y3_conv_workspace_bytes', (3, 13, 13, 64, 0, 128, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (3, 13, 13, 64, 0, 128, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (3, 13, 13, 64, 0, 128, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (2, 8, 8, 64, 0, 128, 3, 1), (0,), 0, 1),
    ('y3_conv_workspace_bytes', (2, 8, 8, 64, 0, 128, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (2, 8, 8, 64, 0, 128, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (2, 8, 8, 64, 0, 128, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (1, 3, 43, 64, 0, 128, 3, 1), (0,), 0, 2),
    ('y3_conv_workspace_bytes', (1, 3, 43, 64, 0, 128, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (1, 3, 43, 64, 0, 128, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (1, 3, 43, 64, 0, 128, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (8, 52, 52, 128, 0, 256, 3, 1), (0,), 0, 169),
    ('y3_conv_workspace_bytes', (8, 52, 52, 128, 0, 256, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (8, 52, 52, 128, 0, 256, 3, 1), (0, 1), 0, 1),
    ('y3_conv_schedule', (8, 52, 52, 128, 0, 256, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 37, 37, 64, 0, 128, 3, 1), (0,), 0, 33),
    ('y3_conv_workspace_bytes', (3, 37, 37, 64, 0, 128, 3, 1), (), 0, 33556480),
    ('y3_conv_schedule', (3, 37, 37, 64, 0, 128, 3, 1), (0, 1), 0, 1),
    ('y3_conv_schedule', (3, 37, 37, 64, 0, 128, 3, 1), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (2, 90, 92, 256, 0, 128, 3, 2), (0,), 0, 33),
    ('y3_conv_workspace_bytes', (2, 90, 92, 256, 0, 128, 3, 2), (), 0, 33556480),
    ('y3_conv_schedule', (2, 90, 92, 256, 0, 128, 3, 2), (0, 1), 0, 1),
    ('y3_conv_schedule', (2, 90, 92, 256, 0, 128, 3, 2), (0, 0), 0, 0),
    ('y3_conv_stats_blocks', (3, 27, 51, 32, 0, 1024, 1, 1), (0,), 0, 65),
    ('y3_conv_workspace_bytes', (3, 27, 51, 32, 0, 1024, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (3, 27, 51, 32, 0, 1024, 1, 1), (0, 1), 0, 2),
    ('y3_conv_schedule', (3, 27, 51, 32, 0, 1024, 1, 1), (0, 0), 0, 2),
    ('y3_conv_stats_blocks', (2, 128, 130, 64, 32, 128, 1, 1), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (2, 128, 130, 64, 32, 128, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (2, 128, 130, 64, 32, 128, 1, 1), (0, 1), 0, 2),
    ('y3_conv_schedule', (2, 128, 130, 64, 32, 128, 1, 1), (0, 0), 0, 2),
    ('y3_conv_stats_blocks', (4, 64, 65, 32, 0, 255, 1, 1), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (4, 64, 65, 32, 0, 255, 1, 1), (), 0, 0),
    ('y3_conv_schedule', (4, 64, 65, 32, 0, 255, 1, 1), (0, 1), 0, 2),
    ('y3_conv_schedule', (4, 64, 65, 32, 0, 255, 1, 1), (0, 0), 0, 2),
    ('y3_conv_stats_blocks', (32, 52, 52, 3, 0, 32, 3, 1), (0,), 0, 0),
    ('y3_conv_workspace_bytes', (32, 52, 52, 3, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_schedule', (32, 52, 52, 3, 0, 32, 3, 1), (0, 1), 0, 0),
    ('y3_conv_schedule', (32, 52, 52, 3, 0, 32, 3, 1), (0, 0), 0, 0),
    ('y3_conv_dgrad_bn_blocks', (3, 20, 28, 128, 0, 64, 1, 1), (), 0, 27),
    ('y3_conv_dgrad_bn_blocks', (3, 20, 28, 128, 0, 128, 1, 1), (), 0, 27),
    ('y3_conv_dgrad_bn_blocks', (3, 20, 28, 64, 0, 128, 1, 1), (), 0, 14),
    ('y3_conv_dgrad_bn_blocks', (3, 20, 28, 32, 0, 64, 1, 1), (), 0, 14),
    ('y3_conv_stats_blocks', (3, 13, 13, 64, 0, 128, 3, 1), (1,), 0, 3),
    ('y3_conv_stats_blocks', (3, 13, 13, 64, 0, 128, 3, 1), (2,), 0, 3),
    ('y3_conv_train_stats_blocks_bf16', (2, 8, 8, 64, 0, 128, 3, 1), (), 0, 1),
    ('y3_conv_train_stats_blocks_bf16', (1, 3, 43, 64, 0, 128, 3, 1), (), 0, 2),
    ('y3_conv_train_stats_blocks_bf16', (2, 8, 8, 64, 0, 128, 1, 1), (), 0, 1),
    ('y3_conv_train_stats_blocks_bf16', (1, 3, 43, 64, 0, 32, 1, 1), (), 0, 2),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (1, 1), 0, 0),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (1, 0), 0, 0),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (2, 1), 0, 1),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (2, 0), 0, 0),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (4, 1), 0, 1),
    ('y3_conv_schedule', (2, 45, 46, 256, 0, 128, 3, 1), (4, 0), 0, 0),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (1, 1), 0, 1),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (1, 0), 0, 0),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (2, 1), 0, 1),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (2, 0), 0, 0),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (4, 1), 0, 1),
    ('y3_conv_schedule', (4, 45, 46, 256, 0, 128, 3, 1), (4, 0), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (1, 1), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (1, 0), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (2, 1), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (2, 0), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (4, 1), 0, 0),
    ('y3_conv_schedule', (2, 6, 6, 256, 0, 64, 3, 1), (4, 0), 0, 0),
    ('y3_conv_stats_blocks', (8, 52, 52, 128, 0, 256, 3, 1), (0,), 2768897, 170),
    ('y3_conv_schedule', (8, 52, 52, 128, 0, 256, 3, 1), (0, 1), 2768897, 0),
    ('y3_conv_workspace_bytes', (8, 52, 52, 128, 0, 256, 3, 1), (), 2768897, 0),
    ('y3_conv_stats_blocks', (4, 20, 28, 64, 0, 128, 1, 1), (0,), 143361, 36),
    ('y3_conv_schedule', (4, 20, 28, 64, 0, 128, 1, 1), (0, 1), 143361, 0),
    ('y3_conv_workspace_bytes', (4, 20, 28, 64, 0, 128, 1, 1), (), 143361, 0),
    ('y3_conv_stats_blocks', (4, 20, 28, 64, 0, 64, 3, 2), (0,), 71681, 6),
    ('y3_conv_schedule', (4, 20, 28, 64, 0, 64, 3, 2), (0, 1), 71681, 0),
    ('y3_conv_workspace_bytes', (4, 20, 28, 64, 0, 64, 3, 2), (), 71681, 0),
    ('y3_conv_dgrad_bn_blocks', (4, 20, 28, 128, 0, 64, 1, 1), (), 143361, 36),
]


# ---- 6. the host answers of the weight gradients and the train step's workspace -------------------------------------------------
# Same form as HOST_ANSWERS.  Recorded from the library as it stood BEFORE the fp32 weight gradient's size query and launcher
# were moved onto one plan (and the bf16 one's scratch size into its Plan); they are not derived from that code.  Scratch bytes
# of the three kernel families and the Winograd eligibility for: the eight WGRAD shapes; one K-step (one split by construction);
# a Winograd launch of 256 tiles (one split); the stem, small and at six 96 x 416 images; the seven cut launches and the stem's
# three- and eight-range cases of test_conv_ranges_cpu.py under their limits; the five weight-gradient shapes of
# test_train_bf16_kernels_gpu.py.  (The bf16 query only where Cin is a multiple of 32.)
WGRAD_HOST_ANSWERS = [
    ('y3_conv_wgrad_scratch_bytes', (3, 150, 146, 64, 0, 32, 1, 1), (), 0, 3367168),
    ('y3_conv_wgrad_wino_eligible', (3, 150, 146, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (3, 150, 146, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (3, 150, 146, 64, 0, 32, 1, 1), (), 0, 2105344),
    ('y3_conv_wgrad_scratch_bytes', (4, 94, 100, 32, 0, 64, 3, 2), (), 0, 10838272),
    ('y3_conv_wgrad_wino_eligible', (4, 94, 100, 32, 0, 64, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (4, 94, 100, 32, 0, 64, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (4, 94, 100, 32, 0, 64, 3, 2), (), 0, 2727936),
    ('y3_conv_wgrad_scratch_bytes', (8, 26, 26, 256, 0, 255, 1, 1), (), 0, 14884096),
    ('y3_conv_wgrad_wino_eligible', (8, 26, 26, 256, 0, 255, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (8, 26, 26, 256, 0, 255, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (8, 26, 26, 256, 0, 255, 1, 1), (), 0, 5744640),
    ('y3_conv_wgrad_scratch_bytes', (3, 37, 37, 64, 0, 128, 3, 1), (), 0, 12681472),
    ('y3_conv_wgrad_wino_eligible', (3, 37, 37, 64, 0, 128, 3, 1), (), 0, 1),
    ('y3_conv_wgrad_wino_scratch_bytes', (3, 37, 37, 64, 0, 128, 3, 1), (), 0, 20054272),
    ('y3_conv_wgrad_bf16_scratch_bytes', (3, 37, 37, 64, 0, 128, 3, 1), (), 0, 5013504),
    ('y3_conv_wgrad_scratch_bytes', (2, 90, 92, 128, 0, 256, 3, 2), (), 0, 30671104),
    ('y3_conv_wgrad_wino_eligible', (2, 90, 92, 128, 0, 256, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (2, 90, 92, 128, 0, 256, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (2, 90, 92, 128, 0, 256, 3, 2), (), 0, 20054016),
    ('y3_conv_wgrad_scratch_bytes', (3, 61, 67, 128, 0, 64, 1, 1), (), 0, 6291712),
    ('y3_conv_wgrad_wino_eligible', (3, 61, 67, 128, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (3, 61, 67, 128, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (3, 61, 67, 128, 0, 64, 1, 1), (), 0, 1572864),
    ('y3_conv_wgrad_scratch_bytes', (3, 52, 50, 256, 0, 75, 1, 1), (), 0, 9369856),
    ('y3_conv_wgrad_wino_eligible', (3, 52, 50, 256, 0, 75, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (3, 52, 50, 256, 0, 75, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (3, 52, 50, 256, 0, 75, 1, 1), (), 0, 2380800),
    ('y3_conv_wgrad_scratch_bytes', (7, 26, 26, 512, 0, 18, 1, 1), (), 0, 2728192),
    ('y3_conv_wgrad_wino_eligible', (7, 26, 26, 512, 0, 18, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (7, 26, 26, 512, 0, 18, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (7, 26, 26, 512, 0, 18, 1, 1), (), 0, 700416),
    ('y3_conv_wgrad_scratch_bytes', (1, 4, 8, 64, 0, 32, 1, 1), (), 0, 8448),
    ('y3_conv_wgrad_wino_eligible', (1, 4, 8, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (1, 4, 8, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (1, 4, 8, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_scratch_bytes', (1, 16, 4, 1024, 0, 1024, 3, 1), (), 0, 37748992),
    ('y3_conv_wgrad_wino_eligible', (1, 16, 4, 1024, 0, 1024, 3, 1), (), 0, 1),
    ('y3_conv_wgrad_wino_scratch_bytes', (1, 16, 4, 1024, 0, 1024, 3, 1), (), 0, 37748992),
    ('y3_conv_wgrad_bf16_scratch_bytes', (1, 16, 4, 1024, 0, 1024, 3, 1), (), 0, 0),
    ('y3_conv_wgrad_scratch_bytes', (1, 32, 32, 3, 0, 32, 3, 1), (), 0, 14155776),
    ('y3_conv_wgrad_wino_eligible', (1, 32, 32, 3, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (1, 32, 32, 3, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_wgrad_scratch_bytes', (6, 96, 416, 3, 0, 32, 3, 1), (), 0, 14155776),
    ('y3_conv_wgrad_wino_eligible', (6, 96, 416, 3, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (6, 96, 416, 3, 0, 32, 3, 1), (), 0, 0),
    ('y3_conv_wgrad_scratch_bytes', (5, 32, 32, 32, 0, 64, 3, 1), (), 150000, 11796736),
    ('y3_conv_wgrad_wino_eligible', (5, 32, 32, 32, 0, 64, 3, 1), (), 150000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 32, 32, 32, 0, 64, 3, 1), (), 150000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 32, 32, 32, 0, 64, 3, 1), (), 150000, 1474560),
    ('y3_conv_wgrad_scratch_bytes', (5, 48, 32, 32, 0, 64, 3, 2), (), 150000, 4423936),
    ('y3_conv_wgrad_wino_eligible', (5, 48, 32, 32, 0, 64, 3, 2), (), 150000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 48, 32, 32, 0, 64, 3, 2), (), 150000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 48, 32, 32, 0, 64, 3, 2), (), 150000, 589824),
    ('y3_conv_wgrad_scratch_bytes', (5, 48, 32, 64, 0, 32, 1, 1), (), 200000, 1966336),
    ('y3_conv_wgrad_wino_eligible', (5, 48, 32, 64, 0, 32, 1, 1), (), 200000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 48, 32, 64, 0, 32, 1, 1), (), 200000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 48, 32, 64, 0, 32, 1, 1), (), 200000, 245760),
    ('y3_conv_wgrad_scratch_bytes', (5, 32, 32, 256, 0, 128, 1, 1), (), 600000, 20971776),
    ('y3_conv_wgrad_wino_eligible', (5, 32, 32, 256, 0, 128, 1, 1), (), 600000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 32, 32, 256, 0, 128, 1, 1), (), 600000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 32, 32, 256, 0, 128, 1, 1), (), 600000, 2621440),
    ('y3_conv_wgrad_scratch_bytes', (7, 26, 26, 128, 0, 256, 3, 1), (), 400000, 66060544),
    ('y3_conv_wgrad_wino_eligible', (7, 26, 26, 128, 0, 256, 3, 1), (), 400000, 1),
    ('y3_conv_wgrad_wino_scratch_bytes', (7, 26, 26, 128, 0, 256, 3, 1), (), 400000, 35389696),
    ('y3_conv_wgrad_bf16_scratch_bytes', (7, 26, 26, 128, 0, 256, 3, 1), (), 400000, 22413312),
    ('y3_conv_wgrad_scratch_bytes', (5, 20, 28, 32, 0, 64, 3, 2), (), 40000, 1696000),
    ('y3_conv_wgrad_wino_eligible', (5, 20, 28, 32, 0, 64, 3, 2), (), 40000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 20, 28, 32, 0, 64, 3, 2), (), 40000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 20, 28, 32, 0, 64, 3, 2), (), 40000, 221184),
    ('y3_conv_wgrad_scratch_bytes', (5, 26, 26, 256, 0, 255, 1, 1), (), 400000, 28201216),
    ('y3_conv_wgrad_wino_eligible', (5, 26, 26, 256, 0, 255, 1, 1), (), 400000, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (5, 26, 26, 256, 0, 255, 1, 1), (), 400000, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (5, 26, 26, 256, 0, 255, 1, 1), (), 400000, 3655680),
    ('y3_conv_wgrad_scratch_bytes', (6, 96, 416, 3, 0, 32, 3, 1), (), 2555905, 14155776),
    ('y3_conv_wgrad_wino_eligible', (6, 96, 416, 3, 0, 32, 3, 1), (), 2555905, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (6, 96, 416, 3, 0, 32, 3, 1), (), 2555905, 0),
    ('y3_conv_wgrad_scratch_bytes', (64, 512, 512, 3, 0, 32, 3, 1), (), 67108865, 41195520),
    ('y3_conv_wgrad_wino_eligible', (64, 512, 512, 3, 0, 32, 3, 1), (), 67108865, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (64, 512, 512, 3, 0, 32, 3, 1), (), 67108865, 0),
    ('y3_conv_wgrad_scratch_bytes', (2, 20, 28, 64, 0, 32, 1, 1), (), 0, 286976),
    ('y3_conv_wgrad_wino_eligible', (2, 20, 28, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (2, 20, 28, 64, 0, 32, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (2, 20, 28, 64, 0, 32, 1, 1), (), 0, 40960),
    ('y3_conv_wgrad_scratch_bytes', (1, 6, 10, 32, 0, 64, 1, 1), (), 0, 16640),
    ('y3_conv_wgrad_wino_eligible', (1, 6, 10, 32, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (1, 6, 10, 32, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (1, 6, 10, 32, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_scratch_bytes', (2, 13, 13, 64, 0, 192, 3, 1), (), 0, 4866304),
    ('y3_conv_wgrad_wino_eligible', (2, 13, 13, 64, 0, 192, 3, 1), (), 0, 1),
    ('y3_conv_wgrad_wino_scratch_bytes', (2, 13, 13, 64, 0, 192, 3, 1), (), 0, 5751040),
    ('y3_conv_wgrad_bf16_scratch_bytes', (2, 13, 13, 64, 0, 192, 3, 1), (), 0, 884736),
    ('y3_conv_wgrad_scratch_bytes', (2, 26, 26, 64, 0, 128, 3, 2), (), 0, 3244288),
    ('y3_conv_wgrad_wino_eligible', (2, 26, 26, 64, 0, 128, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (2, 26, 26, 64, 0, 128, 3, 2), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (2, 26, 26, 64, 0, 128, 3, 2), (), 0, 589824),
    ('y3_conv_wgrad_scratch_bytes', (2, 25, 41, 128, 0, 64, 1, 1), (), 0, 2130176),
    ('y3_conv_wgrad_wino_eligible', (2, 25, 41, 128, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_wino_scratch_bytes', (2, 25, 41, 128, 0, 64, 1, 1), (), 0, 0),
    ('y3_conv_wgrad_bf16_scratch_bytes', (2, 25, 41, 128, 0, 64, 1, 1), (), 0, 294912),
]

# (dtype, batch, size, second stream on, y3_debug_conv_range_limit in force or 0, y3_net_train_workspace_bytes): all variables
# trainable, 80 classes.  Recorded from the same library.
TRAIN_WORKSPACE_ANSWERS = [
    ('f32', 2, 64, 0, 0, 111795200),
    ('f32', 2, 256, 0, 0, 354845952),
    ('f32', 4, 256, 0, 0, 626124544),
    ('f32', 4, 256, 0, 3000000, 626124544),
    ('f32', 2, 64, 1, 0, 111795200),
    ('f32', 2, 256, 1, 0, 367559936),
    ('f32', 4, 256, 1, 0, 653387520),
    ('f32', 4, 256, 1, 3000000, 653387520),
    ('f32_wino', 2, 64, 0, 0, 141933568),
    ('f32_wino', 2, 256, 0, 0, 365125888),
    ('f32_wino', 4, 256, 0, 0, 626706176),
    ('f32_wino', 4, 256, 0, 3000000, 626706176),
    ('f32_wino', 2, 64, 1, 0, 142179328),
    ('f32_wino', 2, 256, 1, 0, 368271616),
    ('f32_wino', 4, 256, 1, 0, 653969152),
    ('f32_wino', 4, 256, 1, 3000000, 653969152),
    ('f32_bf16x6', 2, 64, 0, 0, 109403136),
    ('f32_bf16x6', 2, 256, 0, 0, 364832000),
    ('f32_bf16x6', 4, 256, 0, 0, 632801024),
    ('f32_bf16x6', 4, 256, 0, 3000000, 632801024),
    ('f32_bf16x6', 2, 64, 1, 0, 109583360),
    ('f32_bf16x6', 2, 256, 1, 0, 365716736),
    ('f32_bf16x6', 4, 256, 1, 0, 655050496),
    ('f32_bf16x6', 4, 256, 1, 3000000, 655050496),
    ('bf16', 2, 64, 0, 0, 42578944),
    ('bf16', 2, 256, 0, 0, 190356736),
    ('bf16', 4, 256, 0, 0, 361496320),
    ('bf16', 4, 256, 0, 3000000, 361496320),
    ('bf16', 2, 64, 1, 0, 42759168),
    ('bf16', 2, 256, 1, 0, 200170752),
    ('bf16', 4, 256, 1, 0, 382435072),
    ('bf16', 4, 256, 1, 3000000, 382435072),
]
