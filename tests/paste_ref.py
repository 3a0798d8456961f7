"""Host restatement of the paste-back of crop tensors (include/sdm.h, "Pasting crops back"; csrc/sdm_align_paste_device.h) in numpy:
float32 positions with every operation rounded, int64 everywhere else.  It knows no box and no ownership: every row is pasted over
the WHOLE frame, one row after the other.

  inverse(M)                              (W 6 float32, degenerate) of a float32 crop -> frame matrix
  flags_at(M, cw, ch, W, H)               the flags of sdm_align_paste_tensor_at
  decode(x, dtype-independent, scale, bias)   tensor elements (... x C) -> 0 ... 255
  paste_row(pix, fmt, M, x, alpha, ...)   one row into pix (H x W x bpp uint8, in place); returns (footprint mask, opacity);
                                          origin=(X0, Y0): pix is a window of the frame that starts at frame pixel (X0, Y0)
  paste(pix, fmt, rows, ...)              rows = [(M, x, alpha), ...] in row order
"""
import numpy as np

import align_ref as A
import align_tensor_ref as T

f32 = np.float32
BPP = {T.GRAY: 1, T.BGR: 3, T.RGB: 3, T.BGRA: 4, T.RGBA: 4}


def inverse(M):
    m = np.asarray(M, f32).reshape(6).astype(np.float64)
    with np.errstate(all="ignore"):
        d = m[0] * m[4] - m[1] * m[3]
        w00, w01, w10, w11 = m[4] / d, -m[1] / d, -m[3] / d, m[0] / d
        w02, w12 = -(w00 * m[2] + w01 * m[5]), -(w10 * m[2] + w11 * m[5])
        W = np.array([w00, w01, w02, w10, w11, w12]).astype(f32)
    return W, not (np.isfinite(m).all() and d != 0 and np.isfinite(W).all())


def flags_at(M, cw, ch, W, H):
    m = np.asarray(M, f32).reshape(6)
    if not np.isfinite(m).all():
        return A.DEGENERATE
    return (A.PARTIAL if A.partial(m, cw, ch, W, H) else 0) | (A.DEGENERATE if inverse(m)[1] else 0)


def as_hwc(x, layout, channels):
    """one row of the tensor as crop_height x crop_width x channels"""
    x = np.asarray(x)
    return np.transpose(x, (1, 2, 0)) if layout == "nchw" else x.reshape(x.shape[0], x.shape[1], channels)


def decode(x, scale, bias):
    """x: ... x C in the tensor's dtype.  uint8: the byte.  Floats: e * scale[c] + bias[c] in float32, 0 for a NaN, clamped, ties to even"""
    if x.dtype == np.uint8:
        return x.astype(np.int64)
    C = x.shape[-1]
    s, b = np.broadcast_to(np.asarray(scale, f32), 3)[:C], np.broadcast_to(np.asarray(bias, f32), 3)[:C]
    with np.errstate(all="ignore"):
        f = (x.astype(f32) * s).astype(f32) + b
        p = np.rint(np.minimum(np.maximum(f, f32(0)), f32(255)))
    return np.where(np.isnan(f), 0, p).astype(np.int64)


def paste_row(pix, fmt, M, x, alpha=None, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0), gray_shift=14,
              origin=(0, 0)):
    """origin = (X0, Y0): pix is the window of the frame whose first pixel is frame pixel (X0, Y0); the positions are those of the TRUE
    frame coordinates, and everything returned has the window's shape"""
    H, Wd = pix.shape[:2]
    W, degenerate = inverse(M)
    none = np.zeros((H, Wd), bool)
    if degenerate:
        return none, np.zeros((H, Wd), np.int64)
    p = decode(as_hwc(x, layout, channels), scale, bias)                   # ch x cw x C
    ch, cw = p.shape[:2]
    X = np.arange(origin[0], origin[0] + Wd, dtype=f32)[None, :]
    Y = np.arange(origin[1], origin[1] + H, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        u = ((W[0] * X + W[1] * Y).astype(f32) + W[2]).astype(f32)
        v = ((W[3] * X + W[4] * Y).astype(f32) + W[5]).astype(f32)
        ok = T.accepted(u, v)
        U = np.floor(np.where(ok, u, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
        V = np.floor(np.where(ok, v, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
    u0, fu, v0, fv = U >> 5, U & 31, V >> 5, V & 31
    foot = ok & (u0 >= -1) & (u0 <= cw - 1) & (v0 >= -1) & (v0 <= ch - 1)
    amap = np.full((ch, cw), 255, np.int64) if alpha is None else np.asarray(alpha, np.uint8).astype(np.int64)
    q, a = np.zeros((H, Wd, p.shape[2]), np.int64), np.zeros((H, Wd), np.int64)
    for dx, dy, w in ((0, 0, (32 - fu) * (32 - fv)), (1, 0, fu * (32 - fv)), (0, 1, (32 - fu) * fv), (1, 1, fu * fv)):
        xx, yy = u0 + dx, v0 + dy
        inside = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        xc, yc = np.clip(xx, 0, cw - 1), np.clip(yy, 0, ch - 1)
        q += w[..., None] * p[yc, xc]
        a += w * np.where(inside, amap[yc, xc], 0)
    q, a = (q + 512) >> 10, np.where(foot, (a + 512) >> 10, 0)
    if channels == 3:
        bgr = q[..., ::-1] if order == "rgb" else q
    else:
        bgr = np.repeat(q, 3, -1)
    if fmt == T.GRAY:
        if channels == 3:
            wb, wg, wr = T.WEIGHTS[gray_shift]
            val = ((bgr[..., 0] * wb + bgr[..., 1] * wg + bgr[..., 2] * wr + (1 << (gray_shift - 1))) >> gray_shift)[..., None]
        else:
            val = bgr[..., :1]
    else:
        val = bgr[..., ::-1] if fmt in (T.RGB, T.RGBA) else bgr
    nb = val.shape[-1]
    old = pix[..., :nb].astype(np.int64)
    new = (a[..., None] * val + (255 - a[..., None]) * old + 127) // 255
    pix[..., :nb] = np.where((a > 0)[..., None], new, old).astype(np.uint8)
    return foot, a


def paste(pix, fmt, rows, **spec):
    """rows: (M, x, alpha) in row order, each reading what the previous one left; returns the per-row (footprint, opacity)"""
    return [paste_row(pix, fmt, M, x, alpha, **spec) for M, x, alpha in rows]
