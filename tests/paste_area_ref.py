"""Host restatement of the filtered paste (include/sdm.h, "Pasting crops back, filtered"; csrc/sdm_align_paste_area_device.h) in numpy, on
top of tests/paste_ref.py (the inverse, the decode, the row with S = 1) and tests/align_area_ref.py (S from s2, the offsets): float32
positions with every operation rounded, int64 everywhere else.  It knows no box, no working footprint and no ownership: every row is
pasted over the WHOLE frame, one row after the other.

  samples(M, mode, max_samples, min_scale)      S of a row, from the float32 W of M
  paste_row(pix, fmt, M, x, alpha, S, ...)      one row into pix (H x W x bpp uint8, in place); returns the opacity a (H x W int64)
  paste(pix, fmt, rows, filter..., **spec)      rows = [(M, x, alpha), ...] in row order; returns [(S, a), ...]
"""
import numpy as np

import align_area_ref as R
import align_tensor_ref as T
import paste_ref as P

f32 = np.float32
BILINEAR, AREA = R.BILINEAR, R.AREA


def s2_of(M):
    W, _ = P.inverse(M)
    with np.errstate(all="ignore"):
        return f32(f32(W[0] * W[0]) + f32(W[3] * W[3]))


def samples(M, mode=AREA, max_samples=16, min_scale=1.0):
    W, degenerate = P.inverse(M)
    return R.samples_of_s2(s2_of(M), mode, max_samples, min_scale, degenerate)


def paste_row(pix, fmt, M, x, alpha=None, S=1, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0), gray_shift=14,
              origin=(0, 0)):
    """origin = (X0, Y0): pix is the window of the frame that starts at frame pixel (X0, Y0), as for paste_ref.paste_row"""
    spec = dict(layout=layout, channels=channels, order=order, scale=scale, bias=bias, gray_shift=gray_shift)
    if S == 1:
        return P.paste_row(pix, fmt, M, x, alpha, origin=origin, **spec)[1]
    H, Wd = pix.shape[:2]
    W, degenerate = P.inverse(M)
    assert not degenerate
    p = P.decode(P.as_hwc(x, layout, channels), scale, bias)                   # ch x cw x C
    ch, cw = p.shape[:2]
    o = R.offsets(S)
    fX = (np.arange(origin[0], origin[0] + Wd, dtype=f32)[None, :, None, None] + o[None, None, None, :]).astype(f32)
    fY = (np.arange(origin[1], origin[1] + H, dtype=f32)[:, None, None, None] + o[None, None, :, None]).astype(f32)
    with np.errstate(all="ignore"):
        u = (((W[0] * fX).astype(f32) + (W[1] * fY).astype(f32)).astype(f32) + W[2]).astype(f32)
        v = (((W[3] * fX).astype(f32) + (W[4] * fY).astype(f32)).astype(f32) + W[5]).astype(f32)
        ok = T.accepted(u, v)
        U = np.floor(np.where(ok, u, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
        V = np.floor(np.where(ok, v, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
    u0, fu, v0, fv = U >> 5, U & 31, V >> 5, V & 31
    amap = np.full((ch, cw), 255, np.int64) if alpha is None else np.asarray(alpha, np.uint8).astype(np.int64)
    q, a = np.zeros(u.shape + (p.shape[2],), np.int64), np.zeros(u.shape, np.int64)
    for dx, dy, w in ((0, 0, (32 - fu) * (32 - fv)), (1, 0, fu * (32 - fv)), (0, 1, (32 - fu) * fv), (1, 1, fu * fv)):
        xx, yy = u0 + dx, v0 + dy
        inside = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        xc, yc = np.clip(xx, 0, cw - 1), np.clip(yy, 0, ch - 1)
        q += w[..., None] * p[yc, xc]
        a += w * np.where(inside, amap[yc, xc], 0)
    n = S * S
    qs, asum = q.sum((2, 3)), a.sum((2, 3))
    assert max(qs.max(initial=0), asum.max(initial=0)) + 512 * n < 2 ** 26 + 2 ** 17
    whole = ok.all((2, 3))                                                     # a refused sub-sample: the row does not touch the pixel
    q, a = (qs + 512 * n) // (1024 * n), np.where(whole, (asum + 512 * n) // (1024 * n), 0)
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
    return a


def paste(pix, fmt, rows, mode=AREA, max_samples=16, min_scale=1.0, **spec):
    """rows: (M, x, alpha) in row order, each reading what the previous one left; returns the per-row (S, opacity)"""
    out = []
    for M, x, alpha in rows:
        S = samples(M, mode, max_samples, min_scale)
        out.append((S, paste_row(pix, fmt, M, x, alpha, S, **spec)))
    return out
