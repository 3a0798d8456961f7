"""Host restatement of sdm_align_crops_tensor (include/sdm.h; csrc/sdm_align_tensor.hip) on top of tests/align_ref.py: the chroma warp
of an NV12 frame, the BT.601 conversion, the channel rules and the element formula, from a given float32 crop -> source matrix.  numpy
float32 operations one at a time (each rounded once), integers in int64 with the int32 range asserted where the device uses int32.

  Frame(fmt, pix, uv=None)                      a source frame on the host: H x W (gray, NV12 luma) or H x W x 3 | 4 uint8; uv: ch x cw x 2
  warped(frame, M, width, height)               the warped pixel of every crop position: (B, G, R) int64 height x width x 3, and its kind
  finish(wp, dtype, layout, channels, ...)      output channels, element formula and layout of one crop
  tensor(frame, M, width, height, **spec)       both
"""
import numpy as np

import align_ref as A

GRAY, BGR, RGB, BGRA, RGBA, NV12 = range(6)
f32 = np.float32
WEIGHTS = {14: (1868, 9617, 4899), 15: (3735, 19235, 9798)}       # (wb, wg, wr) of sdm_upload_images_bgr_u8
INT32 = 2 ** 31


class Frame:
    def __init__(self, fmt, pix, uv=None):
        self.fmt, self.pix, self.uv = fmt, np.asarray(pix, np.uint8), None if uv is None else np.asarray(uv, np.uint8)
        self.h, self.w = self.pix.shape[:2]
        if fmt == NV12:
            assert self.uv.shape == ((self.h + 1) >> 1, (self.w + 1) >> 1, 2), self.uv.shape


def accepted(sx, sy):
    """the 2^20 rule (a NaN position is refused too)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(sx) <= A.MAX_POS) & (np.abs(sy) <= A.MAX_POS)


def warp_at(img, sx, sy, fill):
    """The integer bilinear warp of align_ref.warp at given float32 positions, a tap outside the image reading ``fill``.
    img: H x W x C uint8; returns int64 of sx.shape + (C,), 0 at a refused position."""
    H, W, _ = img.shape
    ok = accepted(sx, sy)
    sxs, sys_ = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
    X = np.floor(sxs * f32(32) + f32(0.5)).astype(np.int64)
    Y = np.floor(sys_ * f32(32) + f32(0.5)).astype(np.int64)
    x0, fx, y0, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        return np.where(inside[..., None], v, fill)

    w00, w10 = ((32 - fx) * (32 - fy))[..., None], (fx * (32 - fy))[..., None]
    w01, w11 = ((32 - fx) * fy)[..., None], (fx * fy)[..., None]
    acc = w00 * tap(x0, y0) + w10 * tap(x0 + 1, y0) + w01 * tap(x0, y0 + 1) + w11 * tap(x0 + 1, y0 + 1)
    return np.where(ok[..., None], (acc + 512) >> 10, 0)


def nv12_terms(Y, U, V):
    """every int32 the device forms in the conversion (int64 here), for the range test: the scaled luma, the four chroma products and
    the three sums before the shift"""
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * 1220542
    u, v = U - 128, V - 128
    terms = [y, 1673527 * v, 852492 * v, 409993 * u, 2116026 * u]
    sums = [y + 2116026 * u + (1 << 19), y - 852492 * v, y - 852492 * v - 409993 * u, y - 852492 * v - 409993 * u + (1 << 19),
            y + 1673527 * v + (1 << 19), y + 2116026 * u, y + 1673527 * v]
    return terms, sums


def nv12_to_bgr(Y, U, V):
    """BT.601 limited range with the constants of OpenCV's COLOR_YUV2BGR_NV12: (B, G, R) int64 in [0, 255], last axis 3"""
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * 1220542
    u, v = U - 128, V - 128
    b = (y + 2116026 * u + (1 << 19)) >> 20
    g = (y - 852492 * v - 409993 * u + (1 << 19)) >> 20
    r = (y + 1673527 * v + (1 << 19)) >> 20
    return np.clip(np.stack(np.broadcast_arrays(b, g, r), -1), 0, 255)


def warped(frame, M, width, height):
    """(kind, (B, G, R) int64 height x width x 3): kind "gray" (the three values are g), "colour" or "nv12" (then [..., 0] of the second
    return value of luma() is Y)"""
    sx, sy = A.positions(M, width, height)
    if frame.fmt == GRAY:
        g = A.warp(frame.pix, M, width, height).astype(np.int64)
        return "gray", np.repeat(g[..., None], 3, -1)
    if frame.fmt in (BGR, RGB, BGRA, RGBA):
        v = A.warp(frame.pix, M, width, height).astype(np.int64)[..., :3]      # alpha is never read
        return "colour", v[..., ::-1] if frame.fmt in (RGB, RGBA) else v
    y = A.warp(frame.pix, M, width, height).astype(np.int64)
    cx, cy = (sx * f32(0.5)).astype(f32), (sy * f32(0.5)).astype(f32)
    uv = warp_at(frame.uv, cx, cy, 128)
    bgr = nv12_to_bgr(y, uv[..., 0], uv[..., 1])
    return "nv12", np.where(accepted(sx, sy)[..., None], bgr, 0)


def luma(frame, M, width, height):
    return A.warp(frame.pix, M, width, height).astype(np.int64)


def element(v, scale, bias, dtype):
    """U8: v.  F32: (float)v * scale + bias, the product rounded, then the sum.  F16: that float32 rounded to nearest even."""
    if dtype == "uint8":
        return np.asarray(v).astype(np.uint8)
    p = np.asarray(v).astype(f32) * f32(scale)
    e = (p + f32(bias)).astype(f32)
    return e if dtype == "float32" else e.astype(np.float16)


def finish(kind, bgr, y, dtype="float16", layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0), gray_shift=14):
    """one crop in its layout (C x H x W or H x W x C) from the warped pixels; y: the luma warp of an NV12 frame (channels == 1)"""
    scale, bias = np.broadcast_to(np.asarray(scale, f32), 3), np.broadcast_to(np.asarray(bias, f32), 3)
    if channels == 3:
        v = bgr[..., ::-1] if order == "rgb" else bgr
    elif kind == "gray":
        v = bgr[..., :1]
    elif kind == "nv12":
        v = y[..., None]
    else:
        wb, wg, wr = WEIGHTS[gray_shift]
        v = ((bgr[..., 0] * wb + bgr[..., 1] * wg + bgr[..., 2] * wr + (1 << (gray_shift - 1))) >> gray_shift)[..., None]
    out = np.stack([element(v[..., c], scale[c], bias[c], dtype) for c in range(channels)], -1)
    return np.ascontiguousarray(np.moveaxis(out, -1, 0)) if layout == "nchw" else out


def tensor(frame, M, width, height, **spec):
    kind, bgr = warped(frame, M, width, height)
    return finish(kind, bgr, luma(frame, M, width, height) if kind == "nv12" else None, **spec)
