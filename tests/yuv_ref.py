"""Host restatement of the YUV colour description (include/sdm.h, "YUV colour description and 10-bit surfaces";
csrc/sdm_yuv_device.h): the Q20 constants of every (matrix, range, depth) derived here from Kr and Kb, the decode and the encode in
int64 with the int32 range asserted, and the 10-bit taps of a P010 frame.

The references of the 8-bit paths are not copied: `substituted(desc)` puts this module's decode in place of
align_tensor_ref.nv12_to_bgr, and its encode in place of paste_nv12_ref.luma_of / chroma_of, for the duration of a `with` block --
align_area_ref, warp_ref, warp_area_ref, paste_nv12_ref, warp_paste_nv12_ref and warp_paste_area_ref call them by module name.  Plain
"nv12" (value 5) substitutes nothing: it is the references as they are.  The 10-bit fetches (rigid, area, warp, area warp) are stated
here on the references' positions, quantisation and sample counts, because the references' own taps are cast to uint8.

  Desc("p010:bt709:full")       base, matrix, full, depth, value (the sdm_frame.format), plain
  decode_constants / encode_constants(matrix, full[, depth])
  decode(desc)(Y, U, V) -> (B, G, R);  luma_of(desc)(q);  chroma_of(desc)(m)
  Frame10(desc, y10, uv10)      a P010 frame on the host: the 10-bit samples (word >> 6)
  rigid / area / warp / warp_area(frame10, ...) -> (kind, bgr, y8): what align_tensor_ref.finish takes
"""
import contextlib

import numpy as np

import align_area_ref as AR
import align_ref as A
import align_tensor_ref as T
import paste_nv12_ref as N
import warp_area_ref as WA
import warp_ref as WR

f32 = np.float32
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MATRIX_BITS = {"bt601": 0x000, "bt709": 0x100, "bt2020": 0x200}
FULL_BIT = 0x1000
BASES = {"nv12": 5, "p010": 7}
DESCRIPTIONS = [(m, full) for m in ("bt601", "bt709", "bt2020") for full in (False, True)]       # the six, in table order
INT32 = 2 ** 31


def q20(c):
    """floor(c * 2^20 + 0.5) of a real coefficient evaluated in double"""
    return int(np.floor(np.float64(c) * 1048576.0 + 0.5))


def decode_constants(matrix, full, depth=8):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    one = float(1 << (depth - 8))
    ys = 255.0 / ((1 << depth) - 1) if full else 255.0 / (219.0 * one)
    cs = 255.0 / ((1 << depth) - 1) if full else 255.0 / (224.0 * one)
    return dict(CY=q20(ys), CVR=q20(2.0 * (1.0 - kr) * cs), CUB=q20(2.0 * (1.0 - kb) * cs), CVG=q20(2.0 * kr * (1.0 - kr) / kg * cs),
                CUG=q20(2.0 * kb * (1.0 - kb) / kg * cs), y0=0 if full else 16 << (depth - 8), c0=1 << (depth - 1))


def encode_constants(matrix, full):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full else (219.0 / 255.0, 224.0 / 255.0)
    return dict(YR=q20(kr * sy), YG=q20(kg * sy), YB=q20(kb * sy), y0=0 if full else 16,
                UB=q20(0.5 * sc), UG=q20(0.5 * kg / (1.0 - kb) * sc), UR=q20(0.5 * kr / (1.0 - kb) * sc),
                VR=q20(0.5 * sc), VG=q20(0.5 * kg / (1.0 - kr) * sc), VB=q20(0.5 * kb / (1.0 - kr) * sc))


class Desc:
    """a format name base[:matrix][:range] as the library reads it"""

    def __init__(self, name):
        base, *parts = name.split(":")
        self.name, self.base = name, base
        self.matrix = parts[0] if parts and parts[0] in KR_KB else "bt601"
        self.full = parts[-1] == "full" if parts else False
        self.depth = 10 if base == "p010" else 8
        self.value = BASES[base] | MATRIX_BITS[self.matrix] | (FULL_BIT if self.full else 0)
        self.plain = self.value == 5                                # SDM_FRAME_NV12 with no flag: the constants it always had


def decode_with(k):
    def fn(Y, U, V):
        Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
        y = np.maximum(Y - k["y0"], 0) * k["CY"]
        u, v = U - k["c0"], V - k["c0"]
        sums = [y + k["CUB"] * u + (1 << 19), y - k["CVG"] * v - k["CUG"] * u + (1 << 19), y + k["CVR"] * v + (1 << 19)]
        assert all(np.abs(s).max(initial=0) < INT32 for s in sums + [y - k["CVG"] * v])
        return np.clip(np.stack(np.broadcast_arrays(*[s >> 20 for s in sums]), -1), 0, 255)
    return fn


def decode(desc):
    """(Y, U, V) of the description's depth -> (B, G, R) int64 in [0, 255], last axis 3"""
    return T.nv12_to_bgr if desc.plain else decode_with(decode_constants(desc.matrix, desc.full, desc.depth))


def luma_with(k):
    def fn(q):
        q = np.asarray(q, np.int64)
        return (k["YR"] * q[..., 2] + k["YG"] * q[..., 1] + k["YB"] * q[..., 0] + (k["y0"] << 20) + (1 << 19)) >> 20
    return fn


def chroma_with(k):
    def fn(m):
        m = np.asarray(m, np.int64)
        b, g, r = m[..., 0], m[..., 1], m[..., 2]
        uq = (k["UB"] * b - k["UG"] * g - k["UR"] * r + (128 << 20) + (1 << 19)) >> 20
        vq = (k["VR"] * r - k["VG"] * g - k["VB"] * b + (128 << 20) + (1 << 19)) >> 20
        return np.clip(uq, 0, 255), np.clip(vq, 0, 255)
    return fn


def luma_of(desc):
    return N.luma_of if desc.plain else luma_with(encode_constants(desc.matrix, desc.full))


def chroma_of(desc):
    return N.chroma_of if desc.plain else chroma_with(encode_constants(desc.matrix, desc.full))


@contextlib.contextmanager
def substituted(desc):
    """the references' conversion functions replaced by the description's for the duration of the block (plain "nv12": nothing)"""
    saved = T.nv12_to_bgr, N.luma_of, N.chroma_of
    if not desc.plain:
        T.nv12_to_bgr, N.luma_of, N.chroma_of = decode(desc), luma_of(desc), chroma_of(desc)
    try:
        yield
    finally:
        T.nv12_to_bgr, N.luma_of, N.chroma_of = saved


# ---- P010 ------------------------------------------------------------------------------------------------------------------------
def luma8(y10):
    """min(255, (Y10 + 2) >> 2): the image set's gray byte and a one-channel tensor's value"""
    return np.minimum(255, (np.asarray(y10, np.int64) + 2) >> 2)


class Frame10:
    """words: H x W uint16 and ch x cw x 2 uint16 as they lie in memory (the sample in bits 15..6, noise below)"""

    def __init__(self, desc, y_words, uv_words):
        self.desc, self.y, self.uv = desc, np.asarray(y_words, np.uint16) >> 6, np.asarray(uv_words, np.uint16) >> 6
        self.h, self.w = self.y.shape
        assert self.uv.shape == ((self.h + 1) >> 1, (self.w + 1) >> 1, 2), self.uv.shape


def _halves(sx, sy):
    with np.errstate(invalid="ignore"):
        return (sx * f32(0.5)).astype(f32), (sy * f32(0.5)).astype(f32)


def rigid(fr, M, width, height):
    sx, sy = A.positions(M, width, height)
    y = T.warp_at(fr.y[..., None], sx, sy, 0)[..., 0]
    uv = T.warp_at(fr.uv, *_halves(sx, sy), 512)
    ok = T.accepted(sx, sy)
    return "nv12", np.where(ok[..., None], decode(fr.desc)(y, uv[..., 0], uv[..., 1]), 0), np.where(ok, luma8(y), 0)


def unrounded(img, sx, sy, fill):
    """align_area_ref.unrounded on 10-bit taps: q = sum of w s at float32 positions, at most 1023 * 1024; 0 where refused"""
    H, W, _ = img.shape
    ok = T.accepted(sx, sy)
    sxs, sys_ = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
    X = np.floor(sxs * f32(32) + f32(0.5)).astype(np.int64)
    Y = np.floor(sys_ * f32(32) + f32(0.5)).astype(np.int64)
    x0, fx, y0, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), fill)

    w00, w10 = ((32 - fx) * (32 - fy))[..., None], (fx * (32 - fy))[..., None]
    w01, w11 = ((32 - fx) * fy)[..., None], (fx * fy)[..., None]
    q = w00 * tap(x0, y0) + w10 * tap(x0 + 1, y0) + w01 * tap(x0, y0 + 1) + w11 * tap(x0 + 1, y0 + 1)
    assert q.max(initial=0) <= 1023 * 1024
    return np.where(ok[..., None], q, 0)


def average(q, axes, n):
    total = q.sum(axes)
    assert total.max(initial=0) + 512 * n < 2 ** 32
    return (total + 512 * n) // (1024 * n)


def area(fr, M, width, height, S):
    sx, sy = AR.positions(M, width, height, S)
    whole = T.accepted(sx, sy).all((2, 3))
    y = average(unrounded(fr.y[..., None], sx, sy, 0), (2, 3), S * S)[..., 0]
    uv = average(unrounded(fr.uv, *_halves(sx, sy), 512), (2, 3), S * S)
    return "nv12", np.where(whole[..., None], decode(fr.desc)(y, uv[..., 0], uv[..., 1]), 0), np.where(whole, luma8(y), 0)


def warp(fr, mats, lab):
    sx, sy = WR.positions(mats, lab)
    ok = T.accepted(sx, sy)
    y = T.warp_at(fr.y[..., None], sx, sy, 0)[..., 0]
    uv = T.warp_at(fr.uv, *_halves(sx, sy), 512)
    return "nv12", np.where(ok[..., None], decode(fr.desc)(y, uv[..., 0], uv[..., 1]), 0), np.where(ok, luma8(y), 0)


def warp_area(fr, mats, lab, samples):
    mats, samples = np.asarray(mats, f32).reshape(-1, 6), np.asarray(samples).reshape(-1, 2)
    h, w = lab.shape
    bgr, y8 = np.zeros((h, w, 3), np.int64), np.zeros((h, w), np.int64)
    for t in np.unique(lab):
        if t == WR.NONE:
            continue
        ii, jj = np.nonzero(lab == t)
        Sx, Sy = int(samples[t, 0]), int(samples[t, 1])
        sx, sy = WA.positions(mats[t], jj, ii, Sx, Sy)
        whole = T.accepted(sx, sy).all((1, 2))
        y = average(unrounded(fr.y[..., None], sx, sy, 0), (1, 2), Sx * Sy)[..., 0]
        uv = average(unrounded(fr.uv, *_halves(sx, sy), 512), (1, 2), Sx * Sy)
        bgr[ii, jj] = np.where(whole[:, None], decode(fr.desc)(y, uv[..., 0], uv[..., 1]), 0)
        y8[ii, jj] = np.where(whole, luma8(y), 0)
    return "nv12", bgr, y8
