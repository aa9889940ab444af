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
