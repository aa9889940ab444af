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
