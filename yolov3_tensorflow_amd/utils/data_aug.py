# coding: utf-8
"""Training augmentations with the reference's `utils.data_aug` interface (mix_up, random_color_distort, random_expand,
random_crop_with_constraints, resize_with_bbox, random_flip, letterbox_resize, bbox_crop, bbox_iou), OpenCV-free: numpy +
PIL on RGB uint8 images.

These feed the train step (the feeder); they are host-side plumbing, not the hot path.  What is held
fixed against the reference (utils/data_aug.py:12-380), and how:
  * the box arithmetic - crop windows, IoU, clipping, flips, canvas offsets, mix-up weights - gives the reference's numbers
    draw for draw: tests/test_feeder_cpu.py replays vectors recorded from the reference module under the same seeds
    (tests/golden/make_aug_golden.py).  That pins the ORDER and the arguments of every random draw below, which is why
    each function says which draws it makes;
  * every function takes explicit generators (`rng`: a numpy RandomState, `prng`: a random.Random) and falls back to the
    process-global ones only when given none, so a feeder worker is reproducible from (seed, epoch, sample index) - the
    reference's tf.data threads share the global generators and are not (utils/data_utils.py:190 says so);
  * the colour jitter works in HSV with OpenCV's units (H in [0,180), S and V in [0,255]); the conversion itself goes
    through PIL's C code (hue rescaled), the exact 8-bit OpenCV definition is kept as rgb_to_hsv_u8 / hsv_to_rgb_u8;
  * cv2.resize with the random interpolation 0..4: INTER_NEAREST and INTER_LINEAR are the exact restatements of
    utils/data_utils.py; INTER_CUBIC / INTER_AREA / INTER_LANCZOS4 map to PIL's BICUBIC / BOX / LANCZOS (no OpenCV here).
"""
from __future__ import division, print_function

import math
import random as _random

import numpy as np

_INF = float('inf')


def _gens(rng, prng):
    """(numpy-style generator, random.Random-style generator), each defaulting to the process-global module."""
    return (np.random if rng is None else rng), (_random if prng is None else prng)


def _with_column(boxes, value):
    """boxes [N, C] with one more column holding `value` (float64, as np.full makes it)."""
    return np.hstack([boxes, np.full((len(boxes), 1), value)])


def mix_up_boxes(bbox1, bbox2, rng=None):
    """The image-free half of mix_up: draws the weight (one draw: rng.beta(1.5, 1.5)) and labels the boxes with it.
    Returns (weight of the first image, boxes [N1+N2, 5])."""
    rng, _ = _gens(rng, None)
    lam = min(1, max(0, rng.beta(1.5, 1.5)))
    return lam, np.vstack([_with_column(bbox1, lam), _with_column(bbox2, 1. - lam)])


def blend(img1, img2, lam):
    """The pixel half of mix_up: lam * img1 + (1 - lam) * img2 in float32 on a black canvas that holds both, as uint8."""
    (h1, w1), (h2, w2) = img1.shape[:2], img2.shape[:2]
    canvas = np.zeros((max(h1, h2), max(w1, w2), 3), np.float32)
    canvas[:h1, :w1] = img1.astype(np.float32) * lam
    canvas[:h2, :w2] += img2.astype(np.float32) * (1. - lam)
    return canvas.astype(np.uint8)


def mix_up(img1, img2, bbox1, bbox2, rng=None):
    """Blend two images on a common top-left-anchored canvas with a Beta(1.5, 1.5) weight (reference
    utils/data_aug.py:12-39).  One draw: rng.beta.
    Returns (uint8 HWC image, boxes [N1+N2, 5] = x_min, y_min, x_max, y_max, weight of the image the box came from)."""
    lam, boxes = mix_up_boxes(bbox1, bbox2, rng)
    return blend(img1, img2, lam), boxes


def bbox_crop(bbox, crop_box=None, allow_outside_center=True):
    """Boxes [N, 4+] re-expressed inside the window crop_box = (x_min, y_min, width, height): clipped to it, shifted to
    its origin, and dropped when nothing is left (or, with allow_outside_center=False, when the centre lies outside).
    A None / 0 entry of crop_box means "unbounded on that side" (reference utils/data_aug.py:42-93)."""
    out = bbox.copy()
    if crop_box is None:
        return out
    if len(crop_box) != 4:
        raise ValueError("Invalid crop_box parameter, requires length 4, given {}".format(str(crop_box)))
    if all(c is None for c in crop_box):
        return out
    x0, y0 = crop_box[0] or 0, crop_box[1] or 0
    origin = np.array((x0, y0))
    far = np.array((x0 + (crop_box[2] or _INF), y0 + (crop_box[3] or _INF)))
    if allow_outside_center:
        keep = np.ones(len(out), dtype=bool)
    else:
        mid = (out[:, :2] + out[:, 2:4]) / 2
        keep = ((origin <= mid) & (mid < far)).all(axis=1)
    out[:, :2] = np.maximum(out[:, :2], origin)
    out[:, 2:4] = np.minimum(out[:, 2:4], far)
    out[:, :2] -= origin
    out[:, 2:4] -= origin
    keep &= (out[:, :2] < out[:, 2:4]).all(axis=1)
    return out[keep]


def bbox_iou(bbox_a, bbox_b, offset=0):
    """Pairwise IoU of two box sets ([N, 4+], [M, 4+]) -> [N, M]; `offset` 1 counts pixels inclusively (reference
    utils/data_aug.py:95-125)."""
    if min(bbox_a.shape[1], bbox_b.shape[1]) < 4:
        raise IndexError("Bounding boxes axis 1 must have at least length 4")

    def area(lo, hi):
        side = hi - lo + offset
        return side[..., 0] * side[..., 1]

    lo = np.maximum(bbox_a[:, None, :2], bbox_b[:, :2])
    hi = np.minimum(bbox_a[:, None, 2:4], bbox_b[:, 2:4])
    overlap = area(lo, hi) * (lo < hi).all(axis=2)
    return overlap / (area(bbox_a[:, :2], bbox_a[:, 2:4])[:, None] + area(bbox_b[:, :2], bbox_b[:, 2:4]) - overlap)


def _iou_min_max(rows, crop):
    """min and max over the boxes of bbox_iou(box, crop) for ONE crop box, in plain Python floats: the same float64
    arithmetic as bbox_iou on a [N,4] float32 array against an int crop, without ~10 numpy calls per trial (the crop loop
    runs up to 300 trials per image)."""
    lo, hi = _INF, -_INF
    cl, ct, cr, cb = crop
    area_b = float((cr - cl) * (cb - ct))
    for x0, y0, x1, y1 in rows:
        tlx, tly = max(x0, cl), max(y0, ct)
        brx, bry = min(x1, cr), min(y1, cb)
        area_i = (brx - tlx) * (bry - tly) * (1.0 if (tlx < brx and tly < bry) else 0.0)
        v = area_i / ((x1 - x0) * (y1 - y0) + area_b - area_i)
        lo, hi = min(lo, v), max(hi, v)
    return lo, hi


_DEFAULT_IOU_BANDS = ((0.1, None), (0.3, None), (0.5, None), (0.7, None), (0.9, None), (None, 1))


def _draw_window(prng, w, h, min_scale, max_scale, max_aspect_ratio):
    """One trial window (x, y, width, height) inside a w x h image, or None for a degenerate one.  Draws, in this order:
    scale ~ U(min_scale, max_scale); aspect ~ U(max(1/R, s^2), min(R, 1/s^2)); then y and x offsets by randrange (the
    offsets are not drawn for a degenerate trial - random.randrange(0) raises in the reference there)."""
    s = prng.uniform(min_scale, max_scale)
    root = math.sqrt(prng.uniform(max(1 / max_aspect_ratio, s * s), min(max_aspect_ratio, 1 / (s * s))))
    win_h, win_w = int(h * s / root), int(w * s * root)
    if h - win_h < 1 or w - win_w < 1:
        return None
    y = prng.randrange(h - win_h)
    x = prng.randrange(w - win_w)
    return x, y, win_w, win_h


def _candidate_windows(prng, rows, w, h, min_scale, max_scale, max_aspect_ratio, bands, max_trial):
    """The trial loop of random_crop_with_constraints: per (floor, ceil) band, up to max_trial windows from _draw_window
    until one whose IoU with EVERY box row lies in the band.  Returns (windows found, None), or (None, window) when there
    are no rows: nothing to constrain, the first proper window is the crop."""
    found = []
    for floor, ceil in bands:
        for _ in range(max_trial):
            win = _draw_window(prng, w, h, min_scale, max_scale, max_aspect_ratio)
            if win is None:
                continue
            if not rows:
                return None, win
            x, y, ww, wh = win
            least, most = _iou_min_max(rows, (x, y, x + ww, y + wh))
            if floor <= least and most <= ceil:
                found.append(win)
                break
    return found, None


def _candidate_windows_native(prng, rows, w, h, min_scale, max_scale, max_aspect_ratio, bands, max_trial):
    """_candidate_windows in liby3feed.so (y3f_crop_candidates), drawing from prng's own Mersenne Twister state: the same
    windows, and prng left exactly where the Python loop would leave it (tests/test_feed_native.py).  getstate -> search ->
    setstate is not atomic: like any use of one generator from several threads, it needs a generator per thread (the feeder
    gives every sample its own)."""
    import ctypes
    from .. import feed_native
    version, words, gauss = prng.getstate()
    state = np.array(words, dtype=np.uint32)
    boxes = np.array(rows, dtype=np.float64).reshape(-1, 4)
    limits = np.array(bands, dtype=np.float64).reshape(-1, 2)
    windows = np.zeros((max(1, len(limits)), 4), np.int32)
    count = ctypes.c_int32(0)
    feed_native.check(feed_native.lib().y3f_crop_candidates(
        state.ctypes.data, boxes.ctypes.data, len(boxes), int(w), int(h), float(min_scale), float(max_scale),
        float(max_aspect_ratio), limits.ctypes.data, len(limits), int(max_trial), windows.ctypes.data, ctypes.byref(count)))
    prng.setstate((version, tuple(state.tolist()), gauss))
    if count.value < 0:
        return None, tuple(int(v) for v in windows[0])
    return [tuple(int(v) for v in win) for win in windows[:count.value]], None


def random_crop_with_constraints(bbox, size, min_scale=0.3, max_scale=1, max_aspect_ratio=2, constraints=None,
                                 max_trial=50, rng=None, prng=None):
    """SSD-style random crop (reference utils/data_aug.py:128-225).  For each (min_iou, max_iou) band of `constraints`,
    up to max_trial windows are drawn (prng, see _draw_window) until one whose IoU with EVERY box lies in the band; the
    whole image is always a candidate too.  Candidates are then taken in random order (rng.randint) until one keeps at
    least one box centre.  size = (width, height).
    Returns (boxes [M, 4+] in the window's frame, (x_offset, y_offset, width, height))."""
    rng, prng = _gens(rng, prng)
    w, h = size
    rows = [tuple(float(v) for v in b[:4]) for b in bbox]
    bands = [(-_INF if lo is None else lo, _INF if hi is None else hi)
             for lo, hi in (_DEFAULT_IOU_BANDS if constraints is None else constraints)]
    from .. import feed_native
    search = _candidate_windows
    if feed_native.enabled() and hasattr(prng, 'getstate') and max(w, h) < 2 ** 31:      # (any random.Random, or `random`)
        search = _candidate_windows_native
    found, only = search(prng, rows, w, h, min_scale, max_scale, max_aspect_ratio, bands, max_trial)
    if found is None:
        return bbox, only
    pool = [(0, 0, w, h)] + found
    while pool:
        win = pool.pop(rng.randint(0, len(pool)))
        kept = bbox_crop(bbox, win, allow_outside_center=False)
        if kept.size:
            return kept, tuple(win)
    return bbox, (0, 0, w, h)


def rgb_to_hsv_u8(img):
    """cv2.cvtColor(uint8 RGB -> HSV): H = hue / 2 in [0,180), S = 255 * (V - min) / V, V = max, rounded to uint8."""
    v = img.astype(np.float32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    vmax = v.max(axis=-1)
    vmin = v.min(axis=-1)
    diff = vmax - vmin
    s = np.where(vmax > 0, diff * 255.0 / np.maximum(vmax, 1e-12), 0.0)
    d = np.where(diff > 0, diff, 1.0)
    h = np.where(vmax == r, (g - b) / d, np.where(vmax == g, 2.0 + (b - r) / d, 4.0 + (r - g) / d)) * 60.0
    h = np.where(diff > 0, h, 0.0)
    h = np.where(h < 0, h + 360.0, h) * 0.5
    out = np.stack([np.rint(h) % 180, np.rint(s), vmax], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def hsv_to_rgb_u8(hsv):
    """cv2.cvtColor(uint8 HSV -> RGB), the inverse of rgb_to_hsv_u8 (H in [0,180))."""
    x = hsv.astype(np.float32)
    h, s, v = x[..., 0] * 2.0 / 60.0, x[..., 1] / 255.0, x[..., 2]
    i = np.floor(h).astype(np.int32) % 6
    f = h - np.floor(h)
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.clip(np.rint(np.stack([r, g, b], axis=-1)), 0, 255).astype(np.uint8)


def color_distort_draws(brightness_delta=32, hue_vari=18, sat_vari=0.5, val_vari=0.5, rng=None):
    """The draws of random_color_distort, all from rng, in this order: a coin and, on heads, an integer-truncated
    brightness shift U(-brightness_delta, brightness_delta); one randint(0, 2) choosing the channel order (1: value,
    saturation, hue; 0: saturation, hue, value); then per channel a coin and, on heads, its amount - hue: an integer
    rotation randint(-hue_vari, hue_vari) on the 180-degree circle; saturation / value: a gain 1 + U(-vari, vari).
    Returns (brightness shift, hue rotation or None, saturation gain or None, value gain or None)."""
    rng, _ = _gens(rng, None)
    shift = int(rng.uniform(-brightness_delta, brightness_delta)) if rng.uniform(0, 1) > 0.5 else 0
    amount = [None, None, None]           # hue, saturation, value
    for channel in ((2, 1, 0) if rng.randint(0, 2) else (1, 0, 2)):
        if not rng.uniform(0, 1) > 0.5:
            continue
        if channel == 0:
            amount[0] = int(rng.randint(-hue_vari, hue_vari))
        else:
            vari = (sat_vari, val_vari)[channel - 1]
            amount[channel] = float(1 + rng.uniform(-vari, vari))
    return shift, amount[0], amount[1], amount[2]


def apply_color_distort(img, draws):
    """The pixel half of random_color_distort for draws = (brightness shift, hue rotation, saturation gain, value gain)."""
    from PIL import Image
    shift, hue, sat, val = draws
    if shift:
        img = img.astype(np.float32) + shift
    img = np.clip(img, 0, 255).astype(np.uint8)
    # RGB <-> HSV through PIL's C conversion (hue on a 0..255 circle there: rescaled to OpenCV's 0..180 so that the jitter
    # amounts mean what they mean in the reference); rgb_to_hsv_u8 / hsv_to_rgb_u8 above are the exact 8-bit OpenCV
    # definition in numpy, 10x slower - half of a feeder worker's time per image when they were used here
    hsv = np.asarray(Image.fromarray(img).convert('HSV')).astype(np.float32)
    hsv[..., 0] *= 180.0 / 255.0
    if hue is not None:
        hsv[..., 0] = (hsv[..., 0] + hue) % 180
    if sat is not None:
        hsv[..., 1] *= sat
    if val is not None:
        hsv[..., 2] *= val
    hsv = np.clip(hsv, 0, 255)
    hsv[..., 0] = np.minimum(hsv[..., 0] * (255.0 / 180.0), 255.0)
    return np.asarray(Image.fromarray(hsv.astype(np.uint8), 'HSV').convert('RGB'))


def random_color_distort(img, brightness_delta=32, hue_vari=18, sat_vari=0.5, val_vari=0.5, rng=None):
    """Photometric jitter of an RGB uint8 HWC image: brightness, then hue / saturation / value (reference
    utils/data_aug.py:228-271, which holds BGR: only the conversion differs).  The draws: color_distort_draws."""
    return apply_color_distort(img, color_distort_draws(brightness_delta, hue_vari, sat_vari, val_vari, rng))


def _resize_any(img, new_width, new_height, interp):
    """cv2.resize with interpolation code 0..4 (see the module docstring); the same bytes from liby3feed.so when the native
    path is on, from the numpy restatements / Pillow otherwise."""
    from .. import feed_native
    if feed_native.enabled():
        return feed_native.resize(img, new_width, new_height, interp)
    from .data_utils import resize_nearest_cv2, resize_bilinear_cv2
    if interp == 0:
        return resize_nearest_cv2(img, new_width, new_height)
    if interp == 1:
        return resize_bilinear_cv2(img, new_width, new_height)
    from PIL import Image
    mode = {2: Image.BICUBIC, 3: Image.BOX, 4: Image.LANCZOS}[int(interp)]
    return np.asarray(Image.fromarray(np.asarray(img, np.uint8)).resize((int(new_width), int(new_height)), mode))


def letterbox_geometry(src_w, src_h, new_width, new_height):
    """(scale, fitted width, fitted height, x padding, y padding) of letterbox_resize for a src_w x src_h image."""
    scale = min(new_width / src_w, new_height / src_h)
    fit_w, fit_h = int(scale * src_w), int(scale * src_h)
    return scale, fit_w, fit_h, int((new_width - fit_w) / 2), int((new_height - fit_h) / 2)


def letterbox_resize(img, new_width, new_height, interp=0):
    """Aspect-preserving resize onto a grey (128) new_height x new_width canvas, centred (reference
    utils/data_aug.py:274-293).  Returns (canvas, scale, x padding, y padding) - what maps a box into the canvas."""
    src_h, src_w = img.shape[:2]
    scale, fit_w, fit_h, pad_x, pad_y = letterbox_geometry(src_w, src_h, new_width, new_height)
    canvas = np.full((new_height, new_width, 3), 128, np.uint8)
    canvas[pad_y:pad_y + fit_h, pad_x:pad_x + fit_w] = _resize_any(img, fit_w, fit_h, interp)
    return canvas, scale, pad_x, pad_y


def resize_boxes(bbox, src_w, src_h, new_width, new_height, letterbox=False):
    """The box half of resize_with_bbox: a float32 copy of bbox ([N, >=4], or a flat list of 4k numbers) mapped from a
    src_w x src_h image into the resized (or letterboxed) one."""
    boxes = np.array(bbox, np.float32)
    if boxes.ndim == 1:
        boxes = boxes.reshape(-1, 4)
    xs, ys = boxes[:, 0:3:2], boxes[:, 1:4:2]          # views: x_min/x_max and y_min/y_max
    if letterbox:
        scale, _, _, pad_x, pad_y = letterbox_geometry(src_w, src_h, new_width, new_height)
        xs *= scale
        xs += pad_x
        ys *= scale
        ys += pad_y
    else:
        xs /= src_w
        xs *= new_width
        ys /= src_h
        ys *= new_height
    return boxes


def resize_with_bbox(img, bbox, new_width, new_height, interp=0, letterbox=False):
    """Resize an image (plain stretch, or letterbox) and carry its boxes along (reference utils/data_aug.py:296-320; any
    of the five cv2 interpolation codes).  bbox: [N, >=4]; columns past the fourth (the mix-up weight) pass through."""
    src_h, src_w = img.shape[:2]
    boxes = resize_boxes(bbox, src_w, src_h, new_width, new_height, letterbox)
    if letterbox:
        return letterbox_resize(img, new_width, new_height, interp)[0], boxes
    return _resize_any(img, new_width, new_height, interp), boxes


def flip_boxes(bbox, width, height, px=0, py=0, rng=None):
    """The box half of random_flip: two draws, always both (rng.uniform(0, 1) for x, then y); the boxes (modified in
    place) of a width x height image are mirrored with it.  Returns (flipped in x?, flipped in y?)."""
    rng, _ = _gens(rng, None)
    in_x = rng.uniform(0, 1) < px
    if in_x:
        bbox[:, [0, 2]] = width - bbox[:, [2, 0]]
    in_y = rng.uniform(0, 1) < py
    if in_y:
        bbox[:, [1, 3]] = height - bbox[:, [3, 1]]
    return in_x, in_y


def random_flip(img, bbox, px=0, py=0, rng=None):
    """Mirror the image left-right with probability px and top-bottom with probability py, boxes (modified in place)
    mirrored with it (reference utils/data_aug.py:323-346).  The draws: flip_boxes."""
    in_x, in_y = flip_boxes(bbox, img.shape[1], img.shape[0], px, py, rng)
    if in_x:
        img = img[:, ::-1]
    if in_y:
        img = img[::-1]
    return np.ascontiguousarray(img), bbox


def expand_boxes(bbox, src_w, src_h, max_ratio=4, keep_ratio=True, prng=None):
    """The box half of random_expand.  Draws from prng: the x ratio U(1, max_ratio), the y ratio (only when keep_ratio is
    false), then the y and the x offset by randint (inclusive); the boxes (modified in place) move by the offset.
    Returns (canvas width, canvas height, x offset, y offset)."""
    _, prng = _gens(None, prng)
    grow_x = prng.uniform(1, max_ratio)
    grow_y = grow_x if keep_ratio else prng.uniform(1, max_ratio)
    big_h, big_w = int(src_h * grow_y), int(src_w * grow_x)
    at_y = prng.randint(0, big_h - src_h)
    at_x = prng.randint(0, big_w - src_w)
    shift = (at_x, at_y)
    bbox[:, :2] += shift
    bbox[:, 2:4] += shift
    return big_w, big_h, at_x, at_y


def random_expand(img, bbox, max_ratio=4, fill=0, keep_ratio=True, prng=None):
    """Place the image at a random position on a `fill`-coloured canvas up to max_ratio times larger, boxes (modified in
    place) shifted with it (reference utils/data_aug.py:349-380).  The draws: expand_boxes."""
    src_h, src_w, channels = img.shape
    big_w, big_h, at_x, at_y = expand_boxes(bbox, src_w, src_h, max_ratio, keep_ratio, prng)
    canvas = np.full((big_h, big_w, channels), fill, dtype=img.dtype)
    canvas[at_y:at_y + src_h, at_x:at_x + src_w] = img
    return canvas, bbox


# ---------------------------------------------------------------------------------------------------------------------
# mosaic: one image cut together from windows of four samples of the same size (the rule: include/yolo355.h, y3_mosaic)
# ---------------------------------------------------------------------------------------------------------------------
def mosaic_tiles(record, w, h):
    """The four tiles of one record (cx, cy, ox0, oy0, .., ox3, oy3) as (tx, ty, tw, th, ox, oy), q = 0..3."""
    cx, cy = int(record[0]), int(record[1])
    return [(cx if q & 1 else 0, cy if q & 2 else 0, w - cx if q & 1 else cx, h - cy if q & 2 else cy,
             int(record[2 + 2 * q]), int(record[3 + 2 * q])) for q in range(4)]


def mosaic_record_fault(record, w, h):
    """The validity rule of a mosaic record: None, or what is wrong with it."""
    record = [int(v) for v in record]
    if len(record) != 10:
        return 'a record holds ten integers, not %d' % len(record)
    if not 1 <= record[0] <= w - 1:
        return 'cx=%d outside [1, %d]' % (record[0], w - 1)
    if not 1 <= record[1] <= h - 1:
        return 'cy=%d outside [1, %d]' % (record[1], h - 1)
    for q, (_, _, tw, th, ox, oy) in enumerate(mosaic_tiles(record, w, h)):
        if not 0 <= ox <= w - tw:
            return 'ox%d=%d outside [0, %d]' % (q, ox, w - tw)
        if not 0 <= oy <= h - th:
            return 'oy%d=%d outside [0, %d]' % (q, oy, h - th)
    return None


def mosaic_draw(prng, w, h):
    """One mosaic record for a w x h image.  Ten draws from prng (a random.Random), in this order: the centre
    cx = randrange(w // 4, w - w // 4 + 1) and cy likewise from h; then for each tile q = 0..3 the window's offset
    ox = randrange(0, w - tw + 1), oy = randrange(0, h - th + 1)."""
    w, h = int(w), int(h)
    if w < 4 or h < 4:
        raise ValueError("mosaic_draw: a %dx%d image is too small to cut" % (w, h))
    cx = prng.randrange(w // 4, w - w // 4 + 1)
    cy = prng.randrange(h // 4, h - h // 4 + 1)
    record = [cx, cy]
    for _, _, tw, th, _, _ in mosaic_tiles(record + [0] * 8, w, h):
        record.append(prng.randrange(0, w - tw + 1))
        record.append(prng.randrange(0, h - th + 1))
    return record


def mosaic4(images, boxes, labels, counts, records, min_side=2.0, min_visible=0.25):
    """Compose n images from 4n samples of one size: the numpy float32 form of y3_mosaic and its oracle.
    images [4n, h, w, 3], boxes [4n, kmax, 5] = (x0, y0, x1, y1, m), labels [4n, kmax], counts [4n], records [n, 10].
    Output image i takes tile q from sample 4i+q: pixels are copied from the window at (ox_q, oy_q); the sample's boxes are
    clipped to the window, dropped when a clipped side is below min_side or less than min_visible of the box's area is
    left, and shifted to the tile.  Returns (images [n, h, w, 3], boxes [n, 4 * kmax, 5] float32, labels [n, 4 * kmax],
    counts [n]): kept boxes compacted in the order q, k; zero rows behind the count, like collate's padding."""
    images = np.asarray(images)
    boxes = np.asarray(boxes, np.float32)
    labels, counts = np.asarray(labels), np.asarray(counts)
    records = np.asarray(records, np.int64).reshape(-1, 10)
    n = len(records)
    if images.ndim != 4 or images.shape[0] != 4 * n or boxes.ndim != 3 or boxes.shape[0] != 4 * n or boxes.shape[2] != 5:
        raise ValueError("mosaic4: %d records need images [%d, h, w, 3] and boxes [%d, kmax, 5]" % (n, 4 * n, 4 * n))
    h, w = images.shape[1:3]
    kmax = boxes.shape[1]
    labels, counts = labels.reshape(4 * n, kmax), counts.reshape(4 * n)
    f32 = np.float32
    min_side, min_visible = f32(min_side), f32(min_visible)
    out_images = np.empty((n,) + images.shape[1:], images.dtype)
    out_boxes = np.zeros((n, 4 * kmax, 5), np.float32)
    out_labels = np.zeros((n, 4 * kmax), labels.dtype)
    out_counts = np.zeros((n,), counts.dtype)
    for i in range(n):
        fault = mosaic_record_fault(records[i], w, h)
        if fault:
            raise ValueError("mosaic4: image %d: %s" % (i, fault))
        at = 0
        for q, (tx, ty, tw, th, ox, oy) in enumerate(mosaic_tiles(records[i], w, h)):
            s = 4 * i + q
            out_images[i, ty:ty + th, tx:tx + tw] = images[s, oy:oy + th, ox:ox + tw]
            b = boxes[s, :min(max(int(counts[s]), 0), kmax)]
            x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
            wx0, wy0, wx1, wy1 = f32(ox), f32(oy), f32(ox + tw), f32(oy + th)
            a0, b0, a1, b1 = np.maximum(x0, wx0), np.maximum(y0, wy0), np.minimum(x1, wx1), np.minimum(y1, wy1)
            with np.errstate(invalid='ignore', over='ignore'):
                cw, ch = a1 - a0, b1 - b0
                keep = (cw >= min_side) & (ch >= min_side) & (cw * ch >= min_visible * ((x1 - x0) * (y1 - y0)))
                moved = np.stack([(a0 - wx0) + f32(tx), (b0 - wy0) + f32(ty), (a1 - wx0) + f32(tx), (b1 - wy0) + f32(ty),
                                  b[:, 4]], axis=1)
            k = int(keep.sum())
            out_boxes[i, at:at + k] = moved[keep]
            out_labels[i, at:at + k] = labels[s, :len(b)][keep]
            at += k
        out_counts[i] = at
    return out_images, out_boxes, out_labels, out_counts


# ---------------------------------------------------------------------------------------------------------------------
# random affine warp: rotation / zoom / shear / translation of one image and its boxes (the rule: include/yolo355.h, y3_affine)
# ---------------------------------------------------------------------------------------------------------------------
AFFINE_WORDS = ('ia', 'ib', 'ic', 'id', 'ie', 'if', 'fa', 'fb', 'fc', 'fd', 'fe', 'ff')
AFFINE_COEF_MAX, AFFINE_OFFSET_MAX, AFFINE_MAX_SIDE = 1 << 20, 1 << 30, 4096
AFFINE_IDENTITY = (65536, 0, 0, 0, 65536, 0, 0x3f800000, 0, 0, 0, 0x3f800000, 0)


def _f32_bits(v):
    """The bit pattern of float32(v) as a signed 32-bit integer (what a record's words 6-11 hold)."""
    return int(np.asarray(v, np.float32).view(np.int32))


def affine_record(inverse, forward):
    """A record from an inverse map (ia, ib, ic, id, ie, if as floats in SOURCE PIXEL INDEX units: u = ia*x + ib*y + ic gives
    the source pixel index of output pixel index (x, y)) and a forward map (fa .. ff on continuous coordinates): the inverse
    quantised to Q16 with round(v * 65536), the forward cast to float32."""
    return [int(round(float(v) * 65536.0)) for v in inverse] + [_f32_bits(v) for v in forward]


def affine_forward(record):
    """The six float32 of the forward map held by a record's words 6-11."""
    return (np.asarray([int(v) for v in record[6:12]], np.int64) & 0xffffffff).astype(np.uint32).view(np.float32)


def affine_record_fault(record, w=None, h=None):
    """The validity rule of an affine record (and of the image size, where given): None, or what is wrong with it - the word
    by number and name, and the range it has to lie in."""
    record = [int(v) for v in record]
    if len(record) != 12:
        return 'a record holds twelve integers, not %d' % len(record)
    for name, side in (('w', w), ('h', h)):
        if side is not None and not 1 <= int(side) <= AFFINE_MAX_SIDE:
            return '%s=%d outside [1, %d]' % (name, side, AFFINE_MAX_SIDE)
    for j in range(6):
        bound = AFFINE_OFFSET_MAX if j in (2, 5) else AFFINE_COEF_MAX
        if not -bound <= record[j] <= bound:
            return 'word %d, %s=%d outside [%d, %d]' % (j, AFFINE_WORDS[j], record[j], -bound, bound)
    for j in range(6, 12):
        if not -2 ** 31 <= record[j] < 2 ** 32:
            return 'word %d, %s=%d is no 32-bit pattern' % (j, AFFINE_WORDS[j], record[j])
        if (record[j] & 0x7f800000) == 0x7f800000:
            return 'word %d, %s is not finite (bits 0x%08x)' % (j, AFFINE_WORDS[j], record[j] & 0xffffffff)
    return None


def affine_draw(prng, w, h, degrees=0.0, translate=0.0, scale=0.0, shear=0.0):
    """One affine record for a w x h image.  Six draws from prng (a random.Random), in this order: the angle
    prng.uniform(-degrees, degrees) in degrees; the zoom prng.uniform(1 - scale, 1 + scale); the shears
    prng.uniform(-shear, shear) along x and then along y, in degrees; tx = prng.uniform(0.5 - translate, 0.5 + translate) * w
    and ty likewise with h.  In float64, on continuous coordinates (pixel j covers [j, j + 1), as for boxes and mosaic tiles),
    the forward map is A = T(tx, ty) . Shear . (zoom . Rot) . T(-w/2, -h/2) with Rot = [[cos, -sin], [sin, cos]] and
    Shear = [[1, tan(shear x)], [tan(shear y), 1]].  Its closed-form inverse (ia .. if on continuous coordinates) is taken at
    pixel centres: ic -> ic + 0.5 * (ia + ib) - 0.5, if likewise; affine_record quantises it and casts the forward map.  With
    every range zero the record is exactly AFFINE_IDENTITY."""
    w, h = int(w), int(h)
    angle = math.radians(prng.uniform(-degrees, degrees))
    zoom = prng.uniform(1.0 - scale, 1.0 + scale)
    shx = math.tan(math.radians(prng.uniform(-shear, shear)))
    shy = math.tan(math.radians(prng.uniform(-shear, shear)))
    tx = prng.uniform(0.5 - translate, 0.5 + translate) * w
    ty = prng.uniform(0.5 - translate, 0.5 + translate) * h
    c, s = zoom * math.cos(angle), zoom * math.sin(angle)
    # M = Shear . (zoom . Rot);  A = [M | (tx, ty) - M . (w/2, h/2)]
    fa, fb, fd, fe = c + shx * s, shx * c - s, shy * c + s, c - shy * s
    fc, ff = tx - (fa * (0.5 * w) + fb * (0.5 * h)), ty - (fd * (0.5 * w) + fe * (0.5 * h))
    det = fa * fe - fb * fd
    if not abs(det) > 1e-12:
        raise ValueError("affine_draw: the drawn map is singular (zoom %r, shears %r, %r)" % (zoom, shx, shy))
    ia, ib, id_, ie = fe / det, -fb / det, -fd / det, fa / det
    ic, if_ = -(ia * fc + ib * ff), -(id_ * fc + ie * ff)
    ic, if_ = ic + 0.5 * (ia + ib) - 0.5, if_ + 0.5 * (id_ + ie) - 0.5
    return affine_record((ia, ib, ic, id_, ie, if_), [v + 0.0 for v in (fa, fb, fc, fd, fe, ff)])     # (+ 0.0: no -0)


def affine_warp(images, boxes, labels, counts, records, fill, min_side=2.0, min_area=0.1, max_aspect=20.0):
    """Warp n images and their boxes, one record each: the numpy float32 form of y3_affine and its oracle.
    images [n, h, w, 3] float32, boxes [n, kmax, 5] = (x0, y0, x1, y1, m), labels [n, kmax], counts [n], records [n, 12].
    Every output pixel is the bilinear blend of four taps of its image at the Q16 source position (fill outside); every box
    is the clipped bounding box of its four mapped corners, dropped when a side is below min_side, its area below min_area of
    the mapped box's, or one side more than max_aspect times the other.  Returns (images [n, h, w, 3], boxes [n, kmax, 5]
    float32, labels [n, kmax], counts [n]): kept boxes compacted in order, zero rows behind the count."""
    images = np.asarray(images)
    boxes = np.asarray(boxes, np.float32)
    labels, counts = np.asarray(labels), np.asarray(counts)
    records = np.asarray(records, np.int64).reshape(-1, 12)
    n = len(records)
    if images.ndim != 4 or images.shape[0] != n or images.shape[3] != 3 or images.dtype != np.float32 or boxes.ndim != 3 or \
            boxes.shape[0] != n or boxes.shape[2] != 5:
        raise ValueError("affine_warp: %d records need float32 images [%d, h, w, 3] and boxes [%d, kmax, 5]" % (n, n, n))
    h, w = images.shape[1:3]
    kmax = boxes.shape[1]
    labels, counts = labels.reshape(n, kmax), counts.reshape(n)
    f32 = np.float32
    fill, min_side, min_area, max_aspect = f32(fill), f32(min_side), f32(min_area), f32(max_aspect)
    out_images = np.empty_like(images)
    out_boxes = np.zeros((n, kmax, 5), np.float32)
    out_labels = np.zeros((n, kmax), labels.dtype)
    out_counts = np.zeros((n,), counts.dtype)
    xs, ys = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    for i in range(n):
        fault = affine_record_fault(records[i], w, h)
        if fault:
            raise ValueError("affine_warp: image %d: %s" % (i, fault))
        ia, ib, ic, id_, ie, if_ = (int(v) for v in records[i][:6])
        sx, sy = ia * xs + ib * ys + ic, id_ * xs + ie * ys + if_
        u0, v0 = sx >> 16, sy >> 16
        fx, fy = (sx >> 8) & 255, (sy >> 8) & 255
        wx1, wx0 = (fx.astype(f32) / f32(256))[..., None], ((256 - fx).astype(f32) / f32(256))[..., None]
        wy1, wy0 = (fy.astype(f32) / f32(256))[..., None], ((256 - fy).astype(f32) / f32(256))[..., None]

        def src(u, v):
            inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
            return np.where(inside[..., None], images[i][np.clip(v, 0, h - 1), np.clip(u, 0, w - 1)], fill)
        with np.errstate(invalid='ignore', over='ignore'):
            top = wx0 * src(u0, v0) + wx1 * src(u0 + 1, v0)
            bot = wx0 * src(u0, v0 + 1) + wx1 * src(u0 + 1, v0 + 1)
            out_images[i] = wy0 * top + wy1 * bot
        fa, fb, fc, fd, fe, ff = affine_forward(records[i])
        b = boxes[i, :min(max(int(counts[i]), 0), kmax)]
        x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        with np.errstate(invalid='ignore', over='ignore'):
            us = [(fa * x + fb * y) + fc for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
            vs = [(fd * x + fe * y) + ff for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
            a0 = np.minimum(np.minimum(np.minimum(us[0], us[1]), us[2]), us[3])
            a1 = np.maximum(np.maximum(np.maximum(us[0], us[1]), us[2]), us[3])
            b0 = np.minimum(np.minimum(np.minimum(vs[0], vs[1]), vs[2]), vs[3])
            b1 = np.maximum(np.maximum(np.maximum(vs[0], vs[1]), vs[2]), vs[3])
            a0, b0, a1, b1 = np.maximum(a0, f32(0)), np.maximum(b0, f32(0)), np.minimum(a1, f32(w)), np.minimum(b1, f32(h))
            bw, bh = a1 - a0, b1 - b0
            det = np.abs(fa * fe - fb * fd)
            keep = (bw >= min_side) & (bh >= min_side) & (bw * bh >= min_area * (det * ((x1 - x0) * (y1 - y0)))) & \
                (bw <= max_aspect * bh) & (bh <= max_aspect * bw)
        k = int(keep.sum())
        out_boxes[i, :k] = np.stack([a0, b0, a1, b1, b[:, 4]], axis=1)[keep]
        out_labels[i, :k] = labels[i, :len(b)][keep]
        out_counts[i] = k
    return out_images, out_boxes, out_labels, out_counts
