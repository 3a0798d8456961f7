"""The frames of tests/test_gpu_frame_geometry.py: small face pictures inside large or oddly shaped frames, every frame a view into
ONE device buffer of BUF_BYTES bytes of 255 (a frame: dict(w, h, pitch, off, fmt), off = its first byte in the buffer).  Host only:
the case table, the dense host pixels of every frame, the oracle's integer decisions on them and the conditions a case must meet
for its own inputs."""
import functools

import numpy as np

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
