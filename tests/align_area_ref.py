"""Host restatement of sdm_align_crops_tensor_filtered (include/sdm.h, items 2 to 7; csrc/sdm_align_area.hip) on top of
tests/align_ref.py and tests/align_tensor_ref.py: S of a row, the sub-sample offsets and positions, the un-rounded bilinear value of a
sub-sample, the average and the NV12 / channel rules on the averaged values.  numpy float32 operations one at a time, integers in int64.

  samples(M, degenerate, mode, max_samples, min_scale)   S of a row
  offsets(S)                                             o[u] = float32(2u + 1 - S) / float32(2S)
  positions(M, width, height, S)                         float32 sx, sy of every sub-sample: height x width x S (v) x S (u)
  warped(frame, M, width, height, S)                     (kind, (B, G, R) int64 height x width x 3, averaged Y of an NV12 frame or None)
  tensor(frame, M, width, height, S, **spec)             one crop in its layout, through align_tensor_ref.finish
"""
import numpy as np

import align_tensor_ref as T

BILINEAR, AREA = 0, 1
MAX_S = 16
f32 = np.float32


def s2_of(M):
    m = np.asarray(M, f32).reshape(2, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(m[0, 0] * m[0, 0]) + f32(m[1, 0] * m[1, 0]))


def samples_of_s2(s2, mode=AREA, max_samples=MAX_S, min_scale=1.0, degenerate=False):
    """item 2, from s2 = M00^2 + M10^2 (float32)"""
    s2 = f32(s2)
    if mode != AREA or degenerate or not np.isfinite(s2):
        return 1
    with np.errstate(over="ignore"):
        if s2 < f32(f32(min_scale) * f32(min_scale)):
            return 1
    for S in range(1, int(max_samples) + 1):
        if f32(S * S) >= s2:
            return S
    return int(max_samples)


def samples(M, degenerate=False, mode=AREA, max_samples=MAX_S, min_scale=1.0):
    return samples_of_s2(s2_of(M), mode, max_samples, min_scale, degenerate)


def offsets(S):
    """item 3: one correctly rounded float32 division per entry"""
    return (np.arange(S, dtype=np.int64) * 2 + 1 - S).astype(f32) / f32(2 * S)


def positions(M, width, height, S):
    m = np.asarray(M, f32).reshape(2, 3)
    o = offsets(S)
    fj = (np.arange(width, dtype=f32)[None, :, None, None] + o[None, None, None, :]).astype(f32)
    fi = (np.arange(height, dtype=f32)[:, None, None, None] + o[None, None, :, None]).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = ((m[0, 0] * fj).astype(f32) + (m[0, 1] * fi).astype(f32)).astype(f32) + m[0, 2]
        sy = ((m[1, 0] * fj).astype(f32) + (m[1, 1] * fi).astype(f32)).astype(f32) + m[1, 2]
    return sx.astype(f32), sy.astype(f32)


def unrounded(img, sx, sy, fill):
    """item 4: q = w00 p00 + w10 p10 + w01 p01 + w11 p11 per byte position at float32 positions (int64, sx.shape + (C,)); a tap outside
    the image reads ``fill``; 0 where the position is refused"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, _ = img.shape
    ok = T.accepted(sx, sy)
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
    q = w00 * tap(x0, y0) + w10 * tap(x0 + 1, y0) + w01 * tap(x0, y0 + 1) + w11 * tap(x0 + 1, y0 + 1)
    assert q.max(initial=0) <= 255 * 1024
    return np.where(ok[..., None], q, 0)


def average(q, S):
    """item 5 without the refusal: (sum over the S x S sub-samples + 512 S S) // (1024 S S); q: height x width x S x S x C"""
    total = q.sum((2, 3))
    assert total.max(initial=0) + 512 * S * S < 2 ** 26 + 2 ** 17
    return (total + 512 * S * S) // (1024 * S * S)


def warped(frame, M, width, height, S):
    """(kind, (B, G, R) int64 height x width x 3, y): align_tensor_ref.warped with every pixel averaged over its S x S sub-samples; y: the
    averaged luma of an NV12 frame (what channels == 1 gives), None otherwise"""
    sx, sy = positions(M, width, height, S)
    whole = T.accepted(sx, sy).all((2, 3))[..., None]                   # a refused sub-sample zeroes the pixel
    if frame.fmt == T.GRAY:
        g = np.where(whole, average(unrounded(frame.pix, sx, sy, 0), S), 0)
        return "gray", np.repeat(g, 3, -1), None
    if frame.fmt in (T.BGR, T.RGB, T.BGRA, T.RGBA):
        v = np.where(whole, average(unrounded(frame.pix, sx, sy, 0), S), 0)[..., :3]       # alpha is never read
        return "colour", v[..., ::-1] if frame.fmt in (T.RGB, T.RGBA) else v, None
    y = average(unrounded(frame.pix, sx, sy, 0), S)
    cx, cy = (sx * f32(0.5)).astype(f32), (sy * f32(0.5)).astype(f32)
    uv = average(unrounded(frame.uv, cx, cy, 128), S)
    bgr = T.nv12_to_bgr(y[..., 0], uv[..., 0], uv[..., 1])
    return "nv12", np.where(whole, bgr, 0), np.where(whole, y, 0)[..., 0]


def tensor(frame, M, width, height, S, **spec):
    kind, bgr, y = warped(frame, M, width, height, S)
    return T.finish(kind, bgr, y, **spec)
