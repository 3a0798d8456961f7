"""The frames of tests/test_gpu_frame_geometry.py: small face pictures inside large or oddly shaped frames, every frame a view into
ONE device buffer of BUF_BYTES bytes of 255 (a frame: dict(w, h, pitch, off, fmt), off = its first byte in the buffer).  Host only:
the case table, the dense host pixels of every frame, the oracle's integer decisions on them and the conditions a case must meet
for its own inputs.  Below them the paste cases of tests/test_gpu_frame_geometry_paste.py: the rows, tensors and opacity maps that the four
paste kernels write into these frames, their restatement on a window around every row, and the conditions from its changed-byte masks."""
import functools
import itertools

import numpy as np

import align_ref as A
import align_tensor_ref as T
import paste_area_ref as Q
import paste_cases as PC
import paste_nv12_ref as N
import paste_ref as P
import warp_cases as WC
import warp_paste_ref as WP
import warp_ref as WR
from oracle import sdm_oracle as orc
from superviseddescent_amd import ibug, synth

INT_MAX = 2 ** 31 - 1
BUF_BYTES = 2 ** 32 + 2 ** 29                      # 4.5 GiB: two frames can lie more than 2^32 bytes apart inside it
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
HOG = [(1, 5, 6, 4, 0.6), (1, 5, 4, 4, 0.4)]       # (the two-level cascade of test_gpu_frames_device.py)
O_PARAMS = [orc.HoGParam(*p) for p in HOG]
BPP = {"gray": 1, "nv12": 1, "bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4}
FW, FH = 96, 80                                    # the face frame of cases 1, 2, 5 and 7


def frame(w, h, pitch, off, fmt="gray"):
    return dict(w=w, h=h, pitch=pitch, off=off, fmt=fmt)


def extent(f):
    """bytes from the frame's first byte to behind its last pixel (NV12: behind the last chroma byte)"""
    if f["fmt"] == "nv12":
        return (f["h"] + (f["h"] + 1) // 2 - 1) * f["pitch"] + 2 * ((f["w"] + 1) // 2)
    return (f["h"] - 1) * f["pitch"] + f["w"] * BPP[f["fmt"]]


# ---- case 1 and 2: the 96 x 80 face frame behind growing pitches -------------------------------------------------------------------
P_16, P_24 = 1024, 2 ** 18
P_31 = INT_MAX // FH                               # h * pitch just below INT_MAX
P_OVER = INT_MAX // FH + 2                         # h * pitch just above it
# (every frame lies at least 32 of its rows into the buffer, where the buffer's size allows it: a read above the image that lost
#  its range check would then meet 255s, not the memory before the allocation)
CASE1 = {"pitch 1024": frame(FW, FH, P_16, 2 ** 16 + 5), "pitch 2^18": frame(FW, FH, P_24, 2 ** 24 + 6), "pitch to 2^31": frame(FW, FH, P_31, 2 ** 30 + 7)}
CASE2 = frame(FW, FH, P_OVER, 2 ** 30 + 9)
# the largest stride the fused kernels serve (csrc/sdm_capi_internal.h, SDM_FUSED_MAX_STRIDE) under the tallest frame that keeps
# h * pitch <= INT_MAX; faces up to MAXP_OUT rows above and below it: (rows outside) * pitch stays below 2^31, the documented limit
MAX_STRIDE = 2 ** 20
MAXP_W, MAXP_H, MAXP_OUT = 64, 2047, 2000
MAXP = frame(MAXP_W, MAXP_H, MAX_STRIDE, 2 ** 31 + 2 ** 26 + 3)
# ---- case 3 and 4: tall and wide frames ---------------------------------------------------------------------------------------------
TALL_W, TALL_PITCH = 64, 72
TALL = {65535: frame(TALL_W, 65535, TALL_PITCH, 8192 + 1), 65600: frame(TALL_W, 65600, TALL_PITCH, 8192 + 1)}
WIDE_W, WIDE_H = 70000, 96
WIDE = frame(WIDE_W, WIDE_H, WIDE_W + 24, 2 ** 22 + 3)
# ---- case 5: frames far apart; the FIRST of the list at the highest address ----------------------------------------------------------
FAR = [frame(FW, FH, 100, 2 ** 32 + 2 ** 28 + 5), frame(FW, FH, 96, 2 ** 16 + 3), frame(FW, FH, 128, 2 ** 31 + 2 ** 20 + 2)]
FAR_ORDER = np.array([2, 0, 1, 1, 0, 2, 0, 2, 1], np.int32)      # rows -> frames, not the identity
STACK_PITCH = 2 ** 24                              # sdm_set_images_device(n = 3): offset[2] = 2 h stride
STACK = [frame(FW, FH, STACK_PITCH, 2 ** 29 + 2 ** 12 + i * FH * STACK_PITCH) for i in range(3)]
# ---- case 6: the converter; (w, h, format): chunks = ceil(w / 16) h, a workgroup takes 256 of them -----------------------------------
CONV_SIZES = [(5, 3, "rgb"), (256, 16, "bgr"), (17, 2, "bgra"), (16, 257, "rgba"), (64, 3, "bgr"), (272, 64, "rgb"), (3, 1, "rgba"),
              (1920, 8, "bgra"), (33, 7, "bgr"), (3840, 4, "rgba"), (9, 2, "rgb")]
CONV_FAR = frame(8, 260, 2 ** 24, 2 ** 20 + 4, "bgr")      # row * pitch beyond 2^32


def conv_frames():
    """case 6's frames one behind the other after CONV_FAR's first rows, pitches padded by 1 ... 11 bytes; then CONV_FAR"""
    out, at = [], 2 ** 21
    for i, (w, h, fmt) in enumerate(CONV_SIZES):
        pitch = w * BPP[fmt] + i + 1
        off = (at + 3) // 4 * 4 + i % 4
        out.append(frame(w, h, pitch, off, fmt))
        at = off + h * pitch
    assert at < CONV_FAR["off"] + CONV_FAR["pitch"]      # (all of them between CONV_FAR's rows 0 and 1)
    return out + [CONV_FAR]


def chunks(f):
    return -(-f["w"] // 16) * f["h"]


# ---- case 7: NV12 surfaces (the chroma h * pitch bytes behind the luma) and their twins at a small pitch ------------------------------
NV12_24 = frame(FW, FH, P_24, 2 ** 24 + 2, "nv12")
NV12_31 = frame(FW, FH, P_OVER, 2 ** 30 + 6, "nv12")
NV12_TWINS = [frame(FW, FH, 128, 2 ** 12 + 4, "nv12"), frame(FW, FH, 104, 2 ** 15 + 2, "nv12")]


def table():
    """(case, the quantity the row is named after, its value, lo, hi): lo < value <= hi is what the case needs"""
    t = []
    f = CASE1["pitch 1024"]
    t.append(("1", "(h - 1) pitch, pitch 1024", (f["h"] - 1) * f["pitch"], 2 ** 16, 2 ** 24))
    f = CASE1["pitch 2^18"]
    t.append(("1", "(h - 1) pitch, pitch 2^18", (f["h"] - 1) * f["pitch"], 2 ** 24, 2 ** 31))
    f = CASE1["pitch to 2^31"]
    t.append(("1", "h pitch just below INT_MAX", f["h"] * f["pitch"], INT_MAX - f["h"], INT_MAX))
    t.append(("1", "rows to the wrap at that pitch (a face lies further out)", 2 ** 31 // f["pitch"], 0, FAR_OUT_ROWS))
    t.append(("1", "largest stride of the fused kernels", MAXP["pitch"], MAX_STRIDE - 1, MAX_STRIDE))
    t.append(("1", "h pitch at the largest stride", MAXP["h"] * MAXP["pitch"], INT_MAX - MAX_STRIDE, INT_MAX))
    t.append(("1", "(rows outside + a patch) pitch at the largest stride: inside the limit", (MAXP_OUT + 40) * MAXP["pitch"], 2 ** 31 - 2 ** 27, 2 ** 31 - 1))
    t.append(("2", "h pitch just above INT_MAX", CASE2["h"] * CASE2["pitch"], INT_MAX, INT_MAX + 4 * CASE2["h"]))
    t.append(("3", "last height of the fast kernels", TALL[65535]["h"], 65534, 65535))
    t.append(("3", "first heights of the generic kernel", TALL[65600]["h"], 65535, 2 ** 17))
    t.append(("4", "last column", WIDE["w"] - 1, 2 ** 16, 2 ** 17))
    lo = min(f["off"] for f in FAR)
    t.append(("5", "frame 0 - lowest frame", FAR[0]["off"] - lo, 2 ** 32, BUF_BYTES))
    t.append(("5", "frame 2 - lowest frame", FAR[2]["off"] - lo, 2 ** 31, 2 ** 32))
    t.append(("5", "frame 0 is the highest, not the base", FAR[0]["off"] - max(f["off"] for f in FAR[1:]), 0, BUF_BYTES))
    t.append(("5", "offset[2] of the stack", 2 * FH * STACK_PITCH, 2 ** 31, 2 ** 32))
    t.append(("5", "h stride of the stack", FH * STACK_PITCH, 2 ** 24, INT_MAX))
    cf = conv_frames()
    t.append(("6", "chunks of 256 x 16", chunks(cf[1]), 255, 256))
    t.append(("6", "chunks of 16 x 257", chunks(cf[3]), 256, 257))
    t.append(("6", "workgroups of 272 x 64", -(-chunks(cf[5]) // 256), 4, 5))
    t.append(("6", "chunks per row of 272", -(-cf[5]["w"] // 16), 16, 17))
    t.append(("6", "chunks per row of 1920", -(-cf[7]["w"] // 16), 119, 120))
    t.append(("6", "chunks per row of 3840", -(-cf[9]["w"] // 16), 239, 240))
    for i in (0, 2, 4, 6, 8, 10):                                    # frames of one workgroup between and around the large ones
        t.append(("6", "chunks of the small frame %d" % i, chunks(cf[i]), 0, 256))
    t.append(("6", "(h - 1) pitch of the far colour frame", (CONV_FAR["h"] - 1) * CONV_FAR["pitch"], 2 ** 32, BUF_BYTES - CONV_FAR["off"]))
    t.append(("7", "chroma offset behind the luma", NV12_24["h"] * NV12_24["pitch"], 2 ** 24, INT_MAX))
    t.append(("7", "luma plane extent (wide offsets)", NV12_31["h"] * NV12_31["pitch"], INT_MAX, 2 ** 32))
    for f in NV12_TWINS:
        t.append(("7", "twin's plane extent", (f["h"] * 3 // 2) * f["pitch"], 0, 2 ** 16))
    # the paste cases (paste_cases below) write into the frames above; what they add of their own:
    for pitch, fmt in ((P_16, "gray"), (P_24, "bgr"), (P_31, "rgba"), (P_OVER, "bgra"), (MAX_STRIDE, "rgb")):
        t.append(("2" if pitch == P_OVER else "1", "paste: row bytes of %s inside pitch %d" % (fmt, pitch), FW * BPP[fmt], 0, pitch))
    t.append(("3", "paste: a row centred on Y = 65 535.5 at 32 frame rows per crop", 65535.5 + 16, 65536, TALL[65600]["h"]))
    t.append(("4", "paste: |W00| (fw + 1) of the row without a footprint bound", 15.2 * (WIDE_W + 1), 2 ** 20, 2 ** 21))
    t.append(("4", "paste: |W00| (fw + 1) of the row just below", 14.9 * (WIDE_W + 1), 2 ** 20 - 2 ** 14, 2 ** 20 - 1))
    t.append(("4", "paste: float32 spacing at column 65 536 in 1/6 pixel (the S = 3 offsets)", 6 * 2.0 ** -7, 0, 1))
    t.append(("5", "paste: rows per far frame", 2, 1, 2))
    t.append(("7", "paste: odd surface, pixels of the last block column x row", (NV12_ODD["w"] % 2) * (NV12_ODD["h"] % 2), 0, 1))
    t.append(("7", "paste: chroma= before its luma", NV12_UV_BEFORE["off"] - NV12_UV_BEFORE["uv_off"], 2 ** 24, 2 ** 32))
    t.append(("7", "paste: that chroma plane ends before the luma", NV12_UV_BEFORE["off"] - NV12_UV_BEFORE["uv_off"] - (FH // 2) * P_24, 0, 2 ** 32))
    return t


def all_frames():
    return (list(CASE1.values()) + [dict(f, fmt="nv12") for f in CASE1.values()] + [CASE2, MAXP] + list(TALL.values()) + [WIDE] + FAR + STACK + conv_frames() + [NV12_24, NV12_31] + NV12_TWINS)


# ---- host pixels ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic():
    return synth.make_faces(3, seed=404)[0]


FAR_OUT_ROWS = 85                                  # a face of case 1 lies at least this many rows above / below the 80-row frame


@functools.lru_cache(maxsize=None)
def faces():
    """three 80 x 96 cuts of synthetic faces (H x W) and the five boxes whose patches cross every border of such a frame"""
    images = synthetic()
    imgs = [np.ascontiguousarray(images[0][60:140, 50:146]), np.ascontiguousarray(images[1][70:150, 60:156]),
            np.ascontiguousarray(images[2][80:160, 90:186])]
    w, h = FW, FH
    boxes = np.array([(-25, -20, 70, 70), (w - 45, -18, 66, 66), (-22, h - 40, 64, 64), (w - 40, h - 42, 72, 72),
                      (w // 2 - 30, h // 2 - 30, 60, 60)], np.int32)
    return imgs, boxes


def paste_faces(canvas, at):
    """cuts of the synthetic faces written into the noise canvas with their top left corners at `at` ((x, y), clipped to the canvas)"""
    images = synthetic()
    H, W = canvas.shape
    for k, (x, y) in enumerate(at):
        src = images[k % 3][40:200, 40:200]
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + 160, W), min(y + 160, H)
        canvas[y0:y1, x0:x1] = src[y0 - y:y1 - y, x0 - x:x1 - x]


@functools.lru_cache(maxsize=None)
def tall(h):
    """(image h x 64: noise with faces at the top, around row 65 500 and across the last row; boxes)"""
    img = np.random.default_rng(h).integers(0, 256, (h, TALL_W), dtype=np.uint8)
    paste_faces(img, [(-40, -30), (-50, 65420), (-45, h - 90)])
    boxes = np.array([(-25, -20, 70, 70), (19, -18, 66, 66), (2, 30, 60, 60), (0, 32700, 62, 62), (-6, 65470, 60, 60), (4, 65440, 56, 56),
                      (-22, h - 40, 64, 64), (24, h - 42, 72, 72), (6, h - 70, 52, 52)], np.int32)
    return img, boxes


@functools.lru_cache(maxsize=None)
def maxp():
    """(image 2047 x 64: noise with faces across the first and the last row; boxes, two of them MAXP_OUT rows outside)"""
    h = MAXP_H
    img = np.random.default_rng(11).integers(0, 256, (h, MAXP_W), dtype=np.uint8)
    paste_faces(img, [(-40, -30), (-50, 900), (-45, h - 90)])
    boxes = np.array([(-25, -20, 70, 70), (19, -18, 66, 66), (2, 930, 60, 60), (-22, h - 40, 64, 64), (24, h - 42, 72, 72),
                      (2, h + MAXP_OUT - 70, 60, 60), (2, -MAXP_OUT + 10, 60, 60)], np.int32)
    return img, boxes


@functools.lru_cache(maxsize=None)
def wide():
    """(image 96 x 70 000: noise with faces at the left edge, around column 69 950 and across the right edge; boxes)"""
    img = np.random.default_rng(7).integers(0, 256, (WIDE_H, WIDE_W), dtype=np.uint8)
    paste_faces(img, [(-30, -30), (69860, -40), (WIDE_W - 80, -35)])
    boxes = np.array([(-25, 10, 70, 70), (20, 14, 62, 62), (32700, 8, 64, 64), (65500, 12, 60, 60), (69915, 10, 62, 62),
                      (WIDE_W - 40, 6, 70, 70), (WIDE_W - 75, 16, 60, 60), (WIDE_W - 30, -20, 72, 72)], np.int32)
    return img, boxes


def aligned(boxes):
    return np.stack([synth.align_mean(MEAN, tuple(int(v) for v in b)) for b in boxes]).astype(np.float32)


def oracle_level(images, idx, x, level):
    """(feature rows, integer decisions) of the oracle for rows x on host images of any sizes: row r reads images[idx[r]]"""
    x = np.ascontiguousarray(x, np.float32)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    feat = np.empty((len(x), orc.feature_dim(L, O_PARAMS[level])), np.float32)
    dec = np.empty((len(x), 1 + 2 * L), np.int32)
    for im in np.unique(idx):
        rows = np.flatnonzero(idx == im)
        f, d = orc.hog_features_batch(images[im][None], np.zeros(len(rows), np.int32), x[rows], RE, LE, O_PARAMS[level], n_threads=8, want_idx=True)
        feat[rows], dec[rows] = f, d
    return feat, dec


def patches(dec):
    """(x0, y0, x1, y1) of every patch of every row, each N x L: the ROI [cx - h, cx + h) x [cy - h, cy + h) (adaptive_vlhog.hpp:136)"""
    h = dec[:, :1].astype(np.int64)
    cx, cy = dec[:, 1:1 + L].astype(np.int64), dec[:, 1 + L:].astype(np.int64)
    return cx - h, cy - h, cx + h, cy + h


def conditions(dec, sizes, borders, beyond, far=None):
    """What keeps a case from passing by accident, from the oracle's integer decisions.  sizes: (w, h) of each row's image; borders:
    those the case is about, of "left right top bottom"; beyond(x0, y0, x1, y1, w, h) -> bool arrays: the patch has pixels INSIDE the
    image beyond the boundary the case names; far(rows_outside) -> bool arrays, for a case about faces far above and below the image: a
    patch wholly above and one wholly below it must meet it, rows_outside counted to the patch's far edge.  Returns the names of the conditions that are NOT met (empty: the case is sound)."""
    x0, y0, x1, y1 = patches(dec)
    w = np.asarray([s[0] for s in sizes], np.int64)[:, None]
    h = np.asarray([s[1] for s in sizes], np.int64)[:, None]
    overlap = (x1 > 0) & (x0 < w) & (y1 > 0) & (y0 < h)
    inside = (x0 >= 0) & (x1 <= w) & (y0 >= 0) & (y1 <= h)
    cross = {"left": overlap & (x0 < 0), "right": overlap & (x1 > w), "top": overlap & (y0 < 0), "bottom": overlap & (y1 > h)}
    missing = [] if inside.any() else ["a patch wholly inside"]
    missing += ["a patch across the %s border" % b for b in borders.split() if not cross[b].any()]
    if not (overlap & beyond(np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, w), np.minimum(y1, h), w, h)).any():
        missing.append("a patch beyond the boundary")
    if far is not None:
        if not ((y1 <= 0) & far(-y0)).any():
            missing.append("a patch far above the image")
        if not ((y0 >= h) & far(y1 - h)).any():
            missing.append("a patch far below the image")
    return missing


# the detect cases: name -> (host images, boxes, rows -> images, the frames on the device, borders, beyond, far)
def detect_cases():
    imgs, fb = faces()
    cases = {}
    for name, f in CASE1.items():
        bound = {"pitch 1024": 2 ** 16, "pitch 2^18": 2 ** 24, "pitch to 2^31": INT_MAX - 8 * f["pitch"]}[name]
        cases["1 " + name] = ([imgs[0]], fb, np.zeros(5, np.int32), [f], "left right top bottom",
                              lambda x0, y0, x1, y1, w, h, p=f["pitch"], b=bound: (y1 - 1) * p + x1 - 1 > b, None)
    # faces so far above and below the frame of the largest pitch that a 32-bit (row * pitch) wraps back into the plane
    f = CASE1["pitch to 2^31"]
    fb2 = np.concatenate([fb, [(10, FH + FAR_OUT_ROWS + 10, 70, 70), (14, -FAR_OUT_ROWS - 90, 70, 70)]]).astype(np.int32)
    cases["1 rows far outside"] = ([imgs[0]], fb2, np.zeros(7, np.int32), [f], "left right top bottom",
                                   lambda x0, y0, x1, y1, w, h, p=f["pitch"]: (y1 - 1) * p + x1 - 1 > INT_MAX - 8 * p,
                                   lambda rows, p=f["pitch"]: (rows >= FAR_OUT_ROWS) & (rows * p > 2 ** 31))
    img, b = maxp()
    cases["1 largest fused stride"] = ([img], b, np.zeros(len(b), np.int32), [MAXP], "left right top bottom",
                                       lambda x0, y0, x1, y1, w, h: (y1 - 1) * MAX_STRIDE + x1 - 1 > INT_MAX - 8 * MAX_STRIDE,
                                       lambda rows: (rows * MAX_STRIDE > 2 ** 31 - 2 ** 27) & (rows * MAX_STRIDE < 2 ** 31))
    cases["2 over INT_MAX"] = ([imgs[0]], fb, np.zeros(5, np.int32), [CASE2], "left right top bottom",
                               lambda x0, y0, x1, y1, w, h: (y1 - 1) * CASE2["pitch"] + x1 - 1 > INT_MAX - 8 * CASE2["pitch"], None)
    for hh, f in TALL.items():
        img, b = tall(hh)
        cases["3 height %d" % hh] = ([img], b, np.zeros(len(b), np.int32), [f], "left right top bottom",
                                     lambda x0, y0, x1, y1, w, h, hh=hh: y1 - 1 >= min(hh - 1, 65536), None)
    img, b = wide()
    cases["4 width 70000"] = ([img], b, np.zeros(len(b), np.int32), [WIDE], "left right top", lambda x0, y0, x1, y1, w, h: x1 - 1 >= 65536, None)
    bx = np.array([fb[k % 5] for k in range(len(FAR_ORDER))], np.int32)
    cases["5 far apart"] = (imgs, bx, FAR_ORDER, FAR, "left right top bottom", lambda x0, y0, x1, y1, w, h: x1 > x0, None)
    idx3 = np.array([2, 1, 0, 2, 1, 0, 2], np.int32)
    cases["5 stack"] = (imgs, np.array([fb[(2 * k) % 5] for k in range(7)], np.int32), idx3, STACK, "left right top bottom",
                        lambda x0, y0, x1, y1, w, h: (y1 - 1) * STACK_PITCH > 2 ** 24, None)
    return cases


@functools.lru_cache(maxsize=None)
def level0(name):
    """the oracle's level 0 of a detect case (computed once, shared by the host test and the device tests): (x0, features, decisions)"""
    images, boxes, idx, frames, borders, beyond, far = detect_cases()[name]
    x0 = aligned(boxes)
    feat, dec = oracle_level(images, idx, x0, 0)
    return x0, feat, dec


def unmet(name, dec=None):
    images, boxes, idx, frames, borders, beyond, far = detect_cases()[name]
    dec = level0(name)[2] if dec is None else dec
    return conditions(dec, [(frames[i]["w"], frames[i]["h"]) for i in idx], borders, beyond, far)


# ---- case 9: the tracker's motion-compensated initialisation (csrc/sdm_track_motion.hip) on these frames ---------------------------------
# Every stream of a case is stored on the case's pixels; then every image's content moves by MOTION_MOVE times the least common multiple of
# the cell sizes of the streams on it -- a whole number of every such stream's cells -- and the streams are searched there.
MOTION = (8, 1.25, 0)                              # (search, scale, min_gain)
MOTION_MOVE = (2, -1)


def motion_cases():
    """name -> (host images, boxes of the streams, rows -> images, the frames on the device, the borders the case names,
    beyond(X, Y, pitch) -> bool: a tap of the case's kind, the image whose streams must take a non-zero shift or None).  A stream whose face
    is centred outside its image is lost in step 1, stores nothing and is not stepped again."""
    imgs, fb = faces()
    every = "left right top bottom"
    cases = {}
    img, b = tall(65600)
    bx = np.array(list(b[:4]) + [(4, 65535, 56, 56), (-22, 65600 - 60, 64, 64)], np.int32)       # (the last one: a chip across the bottom)
    cases["tall 65600"] = ([img], bx, np.zeros(len(bx), np.int32), [TALL[65600]], every, lambda X, Y, p: Y >= 65536, None)
    img, b = wide()
    bx = np.array(list(b[:5]) + [tuple(b[5]), (20000, -30, 60, 60)], np.int32)           # (the last one: a chip across the top)
    cases["wide"] = ([img], bx, np.zeros(len(bx), np.int32), [WIDE], every, lambda X, Y, p: X >= 65536, None)
    # (no tap inside a frame of 80 rows lies beyond INT_MAX itself where h * pitch just passes it: the last rows, as the detect cases ask)
    for name, f in (("over INT_MAX", CASE2), ("pitch to 2^31", CASE1["pitch to 2^31"])):
        cases[name] = ([imgs[0]], fb, np.zeros(5, np.int32), [f], every, lambda X, Y, p: Y * p + X > INT_MAX - 8 * p, None)
    bx = np.array([fb[k % 5] for k in range(len(FAR_ORDER))], np.int32)
    cases["far apart"] = (imgs, bx, FAR_ORDER, FAR, every, lambda X, Y, p: X >= 0, 0)
    idx3 = np.array([2, 1, 0, 2, 1, 0, 2], np.int32)
    cases["stack"] = (imgs, np.array([fb[(2 * k) % 5] for k in range(7)], np.int32), idx3, STACK, every,
                      lambda X, Y, p: Y * p > 2 ** 24, None)
    return cases


def motion_moved(images, idx, ks):
    """the images of step 2: image j's content moved by MOTION_MOVE x lcm(cell sizes of the streams on j) pixels (what leaves one edge
    comes in at the other); idx, ks: the image and the cell size of every stored stream"""
    out = []
    for j, im in enumerate(images):
        kk = [int(k) for k, i in zip(ks, idx) if i == j]
        step = int(np.lcm.reduce(kk)) if kk else 1
        assert not kk or max(abs(v) for v in MOTION_MOVE) * step <= MOTION[0] * min(kk)      # within every stream's reach
        out.append(np.ascontiguousarray(np.roll(im, (MOTION_MOVE[1] * step, MOTION_MOVE[0] * step), axis=(0, 1))))
    return out


def motion_unmet(name, grids, shifts):
    """What keeps a motion case from passing by accident, from the restatement alone.  grids: stream -> (k, ox, oy) of the stored
    streams; shifts: stream -> the (dx, dy) pixels the restatement's search takes in step 2.  A stored chip with a tap INSIDE its image
    beyond the case's boundary; a chip across each border the case names; a window that starts left of its image (ox - S k < 0) on the
    case's frame of the largest pitch; on the far case a stream of the far frame that takes a non-zero shift; everywhere a stream that
    takes one.  Returns the names of the conditions that are NOT met."""
    import track_motion_ref as R
    images, boxes, idx, frames, borders, beyond, far = motion_cases()[name]
    S = MOTION[0]
    cross = dict(left=False, right=False, top=False, bottom=False)
    deep, negative = False, False
    widest = max(f["pitch"] for f in frames)
    for i, (k, ox, oy) in grids.items():
        f = frames[idx[i]]
        x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + R.C * k, f["w"]), min(oy + R.C * k, f["h"])
        if x1 <= x0 or y1 <= y0:
            continue
        cross["left"] |= ox < 0
        cross["right"] |= ox + R.C * k > f["w"]
        cross["top"] |= oy < 0
        cross["bottom"] |= oy + R.C * k > f["h"]
        deep |= bool(beyond(x1 - 1, y1 - 1, f["pitch"]))
        negative |= f["pitch"] == widest and ox - S * k < 0
    missing = ["a chip across the %s border" % b for b in borders.split() if not cross[b]]
    if not deep:
        missing.append("a stored chip with a tap beyond the boundary")
    if not negative:
        missing.append("a window with a negative first column on the frame of the largest pitch")
    if not any(np.any(np.asarray(s) != 0) for s in shifts.values()):
        missing.append("a stream that takes a non-zero shift")
    if far is not None and not any(np.any(np.asarray(s) != 0) for i, s in shifts.items() if idx[i] == far):
        missing.append("a stream of the far frame that takes a non-zero shift")
    return missing


def motion_plan(name, rows, lost):
    """From the rows and lost masks of step 1 (the device's; aligned(boxes) stands in for them without one): (the restatement after its
    store and search, its motion state of every stream between the two, the streams that go on, the images of step 2, the shifts the
    restatement's search takes there n x 2, the unmet conditions)"""
    import track_motion_ref as R
    images, boxes, idx, frames, borders, beyond, far = motion_cases()[name]
    n = len(boxes)
    ids = np.arange(n)
    ref = R.Motion(n, *MOTION)
    ref.store_step(ids, rows, lost, images, idx)
    stored = ref.get(ids)
    keep = ids[np.asarray(lost) == 0]
    moved = motion_moved(images, idx[keep], ref.grid[keep, 0])
    shifts = ref.search_step(keep, np.ones(len(keep), bool), moved, idx[keep])
    grids = {int(i): tuple(int(v) for v in ref.grid[i]) for i in keep}
    return ref, stored, keep, moved, shifts, motion_unmet(name, grids, {int(i): s for i, s in zip(keep, shifts)})


# ==== the paste cases of tests/test_gpu_frame_geometry_paste.py =========================================================================
# The four kernels that WRITE into the caller's frames -- the rigid, the filtered, the NV12 and the piecewise-affine paste -- on the
# frames above, the format swapped in.  A case: dict(case, family, frames, idx (row -> frame), mats or points, cw, ch, dtype, layout,
# channels, order, gray_shift, x, alpha, filter, borders, beyond).  A frame of these cases may carry uv_off: the UV plane at a place of
# its own.  The restatements run on a WINDOW of the frame around every row (origin=): the window comes from the row's geometry in double
# precision, never from the kernel's box, and the reference's footprint must stay off every window edge that is no frame edge.
FORMATS = {"gray": T.GRAY, "nv12": T.NV12, "bgr": T.BGR, "rgb": T.RGB, "bgra": T.BGRA, "rgba": T.RGBA}
PASTE_COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
FAMILIES = ("rigid", "area", "nv12", "nv12 area", "warp")
AREA_FILTER = (Q.AREA, 16, 1.0)
WINDOW_MARGIN = 16
NV12_ODD = frame(FW - 1, FH - 1, P_24, 2 ** 24 + 2, "nv12")        # the last block column holds 2 x 1 pixels, the last row 1 x 2, the corner 1
NV12_UV_BEFORE = dict(frame(FW, FH, P_24, 2 ** 29 + 2 ** 12 + 1, "nv12"), uv_off=2 ** 28 + 7)      # chroma= 2^28 bytes BEFORE its luma
FACE_CENTRES = [(48, 40), (3, 4), (93, 77), (70, 20), (30, 60)]    # inside; across left and top; across right and bottom; two more
RIGID_SCALES = [0.5, 0.4, 0.45, 0.9, 0.35]                          # crop pixels per frame pixel (W): magnified crops, S = 1
AREA_SCALES = [0.8, 1.7, 2.6, 1.3, 2.2]                             # S = 1, 2, 3, 2, 3 under "area"
ANGLES = [20.0, -35.0, 0.0, 45.0, -10.0]


def paste_tensor(n, cw, ch, dtype, layout, channels, seed):
    """paste_cases.tensor for frames inside a buffer of 255s: decoded values spread over -40 ... 200 (the lower clamp acts), a NaN and a
    negative infinity in every float row, NO positive infinity -- no element decodes above 200"""
    rng = np.random.default_rng(seed)
    shape = (n, channels, ch, cw) if layout == "nchw" else (n, ch, cw, channels)
    if dtype == "uint8":
        return rng.integers(0, 201, shape, dtype=np.uint8)
    val = rng.uniform(-40.0, 200.0, shape)
    s, b = np.asarray(PC.SCALES, np.float64)[:channels], np.asarray(PC.BIASES, np.float64)[:channels]
    bc = (1, channels, 1, 1) if layout == "nchw" else (1, 1, 1, channels)
    x = ((val - b.reshape(bc)) / s.reshape(bc)).astype(PC.NP_DTYPES[dtype])
    flat = x.reshape(n, -1)
    for r in range(n):
        at = rng.choice(flat.shape[1], 2, replace=False)
        flat[r, at] = np.array([np.nan, -np.inf], flat.dtype)
    return x


def paste_alpha(n, cw, ch, seed):
    """n opacity maps whose entries are 0 (one in ten) or at least 64: a blend of a value <= 200 over 255 gives at most 241"""
    rng = np.random.default_rng(seed)
    a = rng.integers(64, 256, (n, ch, cw), dtype=np.uint8)
    a[rng.random(a.shape) < 0.1] = 0
    a[:, 0, 0] = 255
    return a


def sim(cw, ch, s, ang, cx, cy):
    """crop -> frame: s crop pixels per frame pixel, rotated by ang degrees, the crop's centre on frame point (cx, cy)"""
    R = A.similarity(1.0 / s, ang, 0.0, 0.0)[:, :2]
    t = np.array([cx, cy], np.float64) - R @ np.array([(cw - 1) / 2.0, (ch - 1) / 2.0])
    return np.concatenate([R, t[:, None]], 1).astype(np.float32)


def mesh(cw, ch):
    """(landmark indices, template, triangles, labels) of the RCR-22 mesh on a cw x ch crop"""
    idx, t, tri = WC.mesh_rcr22(cw, ch)
    return idx, t, tri, WR.labels(t, tri, cw, ch)


def mesh_points(mats, cw, ch, seed):
    """N x K x 2 float32: the mesh's template through every row's similarity, every landmark moved by up to 0.3 frame pixels"""
    t = mesh(cw, ch)[1]
    rng = np.random.default_rng(seed)
    return np.stack([A.apply(M, t) + rng.uniform(-0.3, 0.3, t.shape) for M in mats]).astype(np.float32)


def paste_case(k, case, family, frames, idx, places, cw, ch, borders, beyond, scales=None, seeds=None, filt=None, angles=None,
               alpha_kind=None):
    """places: (cx, cy) of every row; the scales, angles, the tensor's dtype / layout / channels / order and the kind of opacity map
    (0: none, 1: one for all rows, 2: one per row) turn with the case's number k unless they are given; seeds: of every frame's pixels"""
    dtype, layout, channels, order = PASTE_COMBOS[(5 * k + 1) % len(PASTE_COMBOS)]
    if family.startswith("nv12"):
        channels = 3                                                           # (one channel leaves the UV plane alone)
    area = family.endswith("area")
    scales = scales or (AREA_SCALES if area else RIGID_SCALES)
    mats = np.stack([sim(cw, ch, scales[r % len(scales)], angles[r] if angles else ANGLES[(r + k) % len(ANGLES)], cx, cy)
                     for r, (cx, cy) in enumerate(places)])
    n = len(idx)
    c = dict(k=k, case=case, family=family, frames=frames, idx=list(idx), mats=mats, cw=cw, ch=ch, dtype=dtype, layout=layout,
             channels=channels, order=order, gray_shift=14 + k % 2, x=paste_tensor(n, cw, ch, dtype, layout, channels, 1000 + k),
             alpha=[None, paste_alpha(1, cw, ch, 2000 + k)[0], paste_alpha(n, cw, ch, 3000 + k)][k % 3 if alpha_kind is None else alpha_kind],
             filter=filt or (AREA_FILTER if area else None), borders=borders, beyond=beyond,
             seeds=seeds or [7000 + 10 * k + i for i in range(len(frames))])
    return c


def paste_points(c):
    """a warp case's landmarks N x K x 2, made on first use (the mesh's triangulation needs the library)"""
    if c.get("points") is None:
        c["points"] = mesh_points(c["mats"], c["cw"], c["ch"], 4000 + c["k"])
    return c["points"]


@functools.lru_cache(maxsize=None)
def paste_cases():
    cases, k = {}, 0

    def add(name, *a, **kw):
        nonlocal k
        assert name not in cases
        cases[name] = paste_case(k, name[0], *a, **kw)
        k += 1

    every = "left right top bottom"
    # offsets: the 96 x 80 frame behind growing pitches, a format each; h * pitch > INT_MAX through every family
    offs = [("pitch 1024", "1", CASE1["pitch 1024"], "gray", 2 ** 16, ("rigid", "area", "nv12", "warp")),
            ("pitch 2^18", "1", CASE1["pitch 2^18"], "bgr", 2 ** 24, ("rigid", "area", "warp")),
            ("pitch to 2^31", "1", CASE1["pitch to 2^31"], "rgba", INT_MAX - 8 * P_31, ("rigid", "area", "warp")),
            ("over INT_MAX", "2", CASE2, "bgra", INT_MAX - 8 * P_OVER, FAMILIES)]
    for tag, digit, f, fmt, bound, families in offs:
        for fam in families:
            g = dict(f, fmt="nv12" if fam.startswith("nv12") else fmt)
            crop = (64, 64) if (fam, tag) == ("area", "over INT_MAX") else [(24, 24), (33, 20), (16, 16)][k % 3]
            scales = [0.8, 1.7, 2.6, 20.0, 4.5] if crop == (64, 64) else None      # (S = 1, 2, 3, 16 -- capped --, 5)
            add("%s %s, %s" % (digit, tag, fam), fam, [g], [0] * 5, FACE_CENTRES, crop[0], crop[1], every,
                lambda x, y, off, b=bound: off > b, scales=scales)
    for fam in ("rigid", "area", "warp"):
        places = [(32, 1000), (2, 3), (61, 2044), (30, 40), (34, 2000)]
        add("1 largest stride, %s" % fam, fam, [dict(MAXP, fmt="rgb")], [0] * 5, places, 24, 24, every,
            lambda x, y, off: off > INT_MAX - 8 * MAX_STRIDE)
    # tall: rows around Y = 65 535 / 65 536: one centred on the boundary, one wholly beyond it (or across the last row), one at the top
    for hh, f in TALL.items():
        places = [(32, 65400), (30, 65535.5), (31, 65571) if hh == 65600 else (33, hh - 4), (20, 5), (60, 32700), (4, hh - 3)]
        for fam in ("rigid", "area", "nv12", "warp"):
            g = dict(f, fmt="nv12" if fam == "nv12" else "gray")
            crop = (16, 16) if fam != "warp" else (24, 24)
            sc = [1.7, 2.6, 1.3, 0.8, 2.2, 1.7] if fam == "area" else [0.5, 0.45, 0.6, 0.5, 0.4, 0.5]
            add("3 height %d, %s" % (hh, fam), fam, [g], [0] * 6, places, crop[0], crop[1], every,
                lambda x, y, off, hh=hh: y >= min(hh - 1, 65536), scales=sc)
    # wide: rows around X = 65 536, at the right edge and at the left edge; the filtered case: a row with |W00| (fw + 1) >= 2^20 -- the
    # branch without a footprint bound -- and one just below it
    places = [(30000, 48), (65536, 40), (65580, 50), (WIDE_W - 3, 40), (2, 50), (69000, 5)]
    for fam in ("rigid", "area", "nv12", "warp"):
        g = dict(WIDE, fmt="nv12" if fam == "nv12" else "gray")
        crop, sc, pl, ang = (24, 24), None, places, None
        if fam == "area":
            crop, sc, ang = (64, 64), [1.7, 15.2, 2.6, 0.8, 14.9, 4.5, 14.9], [20.0, 0.0, -35.0, 45.0, 0.0, -10.0, 0.0]
            pl = places + [(40, 30)]                                           # (W scale 14.9 at the left: mu stays below 2^20)
        add("4 width 70000, %s" % fam, fam, [g], [0] * len(pl), pl, crop[0], crop[1], "left right top",
            lambda x, y, off: x >= 65536, scales=sc, angles=ang)
    # far apart: rows interleaved over FAR, two overlapping rows on every frame
    far_idx = [0, 1, 2, 1, 0, 2]
    far_places = [(48, 40), (40, 36), (38, 50), (47, 44), (56, 33), (12, 68)]
    for fam in ("rigid", "area", "nv12", "warp"):
        g = [dict(f, fmt="nv12" if fam == "nv12" else "gray") for f in FAR]
        crop, sc = ((64, 64), [0.8, 1.7, 1.3, 1.3, 2.2, 0.8]) if fam == "area" else ((24, 24), None)
        add("5 far apart, %s" % fam, fam, g, far_idx, far_places, crop[0], crop[1], "left bottom", lambda x, y, off: x >= 0, scales=sc,
            alpha_kind=2)
    # NV12: the far chroma plane and the plane over INT_MAX beside their twins (the same rows on all four); odd sizes; chroma= before luma
    four = [NV12_24, NV12_TWINS[0], NV12_31, NV12_TWINS[1]]
    tw_places = [p for p in FACE_CENTRES[:3] for _ in range(4)]
    for fam in ("nv12", "nv12 area"):
        add("7 twins, %s" % fam, fam, four, [0, 1, 2, 3] * 3, tw_places, 24, 24, every, lambda x, y, off: x >= 0,
            scales=[s for s in ((0.8, 1.7, 2.6) if fam == "nv12 area" else (0.5, 0.4, 0.45)) for _ in range(4)], seeds=[71, 71, 72, 72])
        c = cases["7 twins, %s" % fam]
        c["mats"] = np.repeat(c["mats"][0::4], 4, 0)                           # (the angle turns with the row: the twins get ONE matrix,
        c["x"] = np.repeat(c["x"][0::4], 4, 0)                                 #  one tensor row and one opacity map)
        if c["alpha"] is not None and c["alpha"].ndim == 3:
            c["alpha"] = np.repeat(c["alpha"][0::4], 4, 0)
    add("7 odd surface, nv12 area", "nv12 area", [NV12_ODD], [0] * 5, [(47, 40), (3, 4), (93, 77), (92, 20), (30, 77)], 33, 20, every,
        lambda x, y, off: (x == NV12_ODD["w"] - 1) & (y == NV12_ODD["h"] - 1))
    add("7 chroma before luma, nv12", "nv12", [NV12_UV_BEFORE], [0] * 5, FACE_CENTRES, 24, 24, every, lambda x, y, off: off > 2 ** 24)
    return cases


def paste_pixels(c):
    """what the frames hold before the paste: noise; NV12: (luma, chroma)"""
    out = []
    for f, seed in zip(c["frames"], c["seeds"]):
        rng = np.random.default_rng(seed)
        if f["fmt"] == "nv12":
            out.append((rng.integers(0, 256, (f["h"], f["w"]), dtype=np.uint8),
                        rng.integers(0, 256, ((f["h"] + 1) // 2, (f["w"] + 1) // 2, 2), dtype=np.uint8)))
        else:
            out.append(rng.integers(0, 256, (f["h"], f["w"]) + ((BPP[f["fmt"]],) if BPP[f["fmt"]] > 1 else ()), dtype=np.uint8))
    return out


def paste_placement(c, pixels):
    """(frames, pixels) as test_gpu_frame_geometry.placed takes them: an NV12 frame with a UV plane of its own becomes two gray frames"""
    frames, pix = [], []
    for f, p in zip(c["frames"], pixels):
        if "uv_off" in f:
            cw2, ch2 = 2 * ((f["w"] + 1) // 2), (f["h"] + 1) // 2
            frames += [frame(f["w"], f["h"], f["pitch"], f["off"]), frame(cw2, ch2, f["pitch"], f["uv_off"])]
            pix += [p[0], p[1].reshape(ch2, cw2)]
        else:
            frames.append(dict(f))
            pix.append(p)
    return frames, pix


def paste_spec(c):
    return dict(layout=c["layout"], order=c["order"], scale=PC.SCALES, bias=PC.BIASES, gray_shift=c["gray_shift"])


def paste_window(f, pts, even):
    """(x0, y0, x1, y1): the extremes of the points (float64) widened by WINDOW_MARGIN pixels, clipped to the frame; even: on whole 2 x 2
    blocks (an odd end is the frame's own)"""
    p = np.asarray(pts, np.float64)
    x0, y0 = int(np.floor(p[:, 0].min())) - WINDOW_MARGIN, int(np.floor(p[:, 1].min())) - WINDOW_MARGIN
    x1, y1 = int(np.ceil(p[:, 0].max())) + WINDOW_MARGIN + 1, int(np.ceil(p[:, 1].max())) + WINDOW_MARGIN + 1
    if even:
        x0, y0, x1, y1 = x0 - x0 % 2, y0 - y0 % 2, x1 + x1 % 2, y1 + y1 % 2
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, f["w"]), min(y1, f["h"])
    assert x1 > x0 and y1 > y0
    return x0, y0, x1, y1


def row_window(c, r):
    f = c["frames"][c["idx"][r]]
    if c["family"] == "warp":
        return paste_window(f, paste_points(c)[r], False)
    cw, ch = c["cw"], c["ch"]
    return paste_window(f, A.apply(c["mats"][r], [(0, 0), (cw, 0), (0, ch), (cw, ch)]), c["family"].startswith("nv12"))


def paste_reference(c, pixels, whole=False):
    """The restatement of the case's family on copies of the pixels, every row on its window.  Returns (the frames afterwards, per row
    dict(origin, touched: the footprint or the pixels with an opacity above 0, changed: the pixels with a changed byte, chroma: the
    chroma samples with a changed byte or None, S, a)).  Asserts for every row that `touched` stays off the window's edges that are not
    the frame's.  whole: every row over its WHOLE frame, as the restatements were written (origin (0, 0))."""
    want = [tuple(p.copy() for p in q) if isinstance(q, tuple) else q.copy() for q in pixels]
    spec, fam, info = paste_spec(c), c["family"], []
    if fam == "warp":
        idx, t, tri, lab = mesh(c["cw"], c["ch"])
        wmats = WP.matrices(paste_points(c), t, tri)
    for r, im in enumerate(c["idx"]):
        f = c["frames"][im]
        x0, y0, x1, y1 = (0, 0, f["w"], f["h"]) if whole else row_window(c, r)
        alpha = None if c["alpha"] is None else c["alpha"] if c["alpha"].ndim == 2 else c["alpha"][r]
        S, chroma = 1, None
        if fam.startswith("nv12"):
            Y, UV = want[im][0][y0:y1, x0:x1], want[im][1][y0 // 2:(y1 + 1) // 2, x0 // 2:(x1 + 1) // 2]
            before, cbefore = Y.copy(), UV.copy()
            S = 1 if c["filter"] is None else Q.samples(c["mats"][r], *c["filter"])
            a = N.paste_row(Y, UV, c["mats"][r], c["x"][r], alpha, S, channels=c["channels"], origin=(x0, y0), **spec)
            touched, changed, chroma = a > 0, Y != before, (UV != cbefore).any(-1)
        else:
            pix = (want[im] if want[im].ndim == 3 else want[im][..., None])[y0:y1, x0:x1]      # (a view: H x W x bpp)
            before = pix.copy()
            if fam == "warp":
                touched, a, _ = WP.paste_row(pix, FORMATS[f["fmt"]], paste_points(c)[r], tri, wmats[r], lab, c["x"][r], alpha,
                                             channels=c["channels"], origin=(x0, y0), **spec)
            elif fam == "area":
                S = Q.samples(c["mats"][r], *c["filter"])
                a = Q.paste_row(pix, FORMATS[f["fmt"]], c["mats"][r], c["x"][r], alpha, S, channels=c["channels"], origin=(x0, y0), **spec)
                touched = a > 0
            else:
                touched, a = P.paste_row(pix, FORMATS[f["fmt"]], c["mats"][r], c["x"][r], alpha, channels=c["channels"], origin=(x0, y0),
                                         **spec)
            changed = pix != before
            changed = changed.any(-1) if changed.ndim == 3 else changed
        touched = touched | (a > 0)
        for edge, is_frame_edge in ((touched[:, 0], x0 == 0), (touched[:, -1], x1 == f["w"]), (touched[0], y0 == 0), (touched[-1], y1 == f["h"])):
            assert is_frame_edge or not edge.any(), ("the footprint touches the window's edge", c["family"], r, (x0, y0, x1, y1))
        info.append(dict(origin=(x0, y0), touched=touched, changed=changed, chroma=chroma, S=S, a=a))
    return want, info


@functools.lru_cache(maxsize=None)
def paste_expected(name):
    """(the pixels before, the frames afterwards, the per-row records) of a case: computed once, shared, never written to"""
    c = paste_cases()[name]
    pixels = paste_pixels(c)
    want, info = paste_reference(c, pixels)
    return pixels, want, info


def paste_flags(c):
    if c["family"] == "warp":
        idx, t, tri, lab = mesh(c["cw"], c["ch"])
        return WP.flags(paste_points(c), t, tri, [(c["frames"][i]["w"], c["frames"][i]["h"]) for i in c["idx"]])
    return np.array([P.flags_at(c["mats"][r], c["cw"], c["ch"], c["frames"][i]["w"], c["frames"][i]["h"]) for r, i in enumerate(c["idx"])], np.int32)


def area_magnitudes(M, fw, fh):
    """(mu, mv) of csrc/sdm_align_paste_area_device.h: |W00| (fw + 1) + |W01| (fh + 1) + |W02| and the same of W's second row, in double
    on the float32 W"""
    W = P.inverse(M)[0].astype(np.float64)
    return (abs(W[0]) * (fw + 1.0) + abs(W[1]) * (fh + 1.0) + abs(W[2]), abs(W[3]) * (fw + 1.0) + abs(W[4]) * (fh + 1.0) + abs(W[5]))


def paste_unmet(name, rows=None):
    """What keeps a paste case from passing by accident, from the restatement's changed-byte masks, in the style of conditions(): a row
    wholly inside its frame that changes bytes; a row that changes a pixel ON each border the case names (and is PARTIAL); a changed byte
    beyond the boundary the case names (beyond(x, y, byte offset of the pixel inside its frame); an NV12 case with a far chroma plane: a
    changed chroma byte more than 2^24 bytes behind the luma's first); on FAR a pixel under two rows with 0 < a < 255; the wide filtered
    case: mu >= 2^20 for one row and mu, mv < 2^20 for another row with S > 1.  rows: only these rows count (None: all).  Returns the
    names of the conditions that are NOT met."""
    c = paste_cases()[name]
    info = paste_expected(name)[2]
    rows = range(len(c["idx"])) if rows is None else rows
    partial = paste_flags(c) & A.PARTIAL != 0
    inside, beyond, far_chroma, on = False, False, False, dict(left=False, right=False, top=False, bottom=False)
    under = {}
    for r in rows:
        f, rec = c["frames"][c["idx"][r]], info[r]
        ys, xs = np.nonzero(rec["changed"])
        xs, ys = xs + rec["origin"][0], ys + rec["origin"][1]
        if xs.size == 0:
            continue
        inside |= not partial[r]
        if partial[r]:
            on["left"] |= bool((xs == 0).any())
            on["right"] |= bool((xs == f["w"] - 1).any())
            on["top"] |= bool((ys == 0).any())
            on["bottom"] |= bool((ys == f["h"] - 1).any())
        beyond |= bool(np.any(c["beyond"](xs, ys, ys * f["pitch"] + xs * BPP[f["fmt"]])))
        if rec["chroma"] is not None and rec["chroma"].any():
            cy, cx = np.nonzero(rec["chroma"])
            uv0 = f.get("uv_off", f["off"] + f["h"] * f["pitch"]) - f["off"]
            far_chroma |= bool((np.abs(uv0 + (cy + rec["origin"][1] // 2) * f["pitch"] + 2 * (cx + rec["origin"][0] // 2)) > 2 ** 24).any())
        ay, ax = np.nonzero((rec["a"] > 0) & (rec["a"] < 255))
        seen = under.setdefault(c["idx"][r], [set(), False])                   # (the frame's blended pixels so far, one under two rows)
        pts = set(zip((ax + rec["origin"][0]).tolist(), (ay + rec["origin"][1]).tolist()))
        seen[1] |= bool(seen[0] & pts)
        seen[0] |= pts
    missing = [] if inside else ["a row wholly inside"]
    missing += ["a row across the %s border" % b for b in c["borders"].split() if not on[b]]
    if not beyond:
        missing.append("a changed byte beyond the boundary")
    if c["family"].startswith("nv12") and c["case"] == "7" and "twins" in name and not far_chroma:
        missing.append("a changed chroma byte beyond 2^24")
    if c["case"] == "5" and not all(v[1] for v in under.values()):
        missing.append("a pixel under two rows with 0 < a < 255 on every frame")
    if name == "4 width 70000, area":
        f = c["frames"][0]
        mag = [area_magnitudes(c["mats"][r], f["w"], f["h"]) + (info[r]["S"],) for r in rows]
        if not any(mu >= 2 ** 20 and S > 1 for mu, mv, S in mag):
            missing.append("a filtered row with mu >= 2^20")
        if not any(2 ** 20 - 2 ** 14 < mu < 2 ** 20 and mv < 2 ** 20 and S > 1 for mu, mv, S in mag):
            missing.append("a filtered row with mu just below 2^20")
    return missing
