"""Host restatement of the filtered piecewise-affine paste (include/sdm.h, "Pasting warped faces back, filtered";
csrc/sdm_warp_paste_area_device.h) in numpy, on top of tests/warp_paste_ref.py (the box, the triangle map, W_t), tests/paste_area_ref.py
and tests/align_area_ref.py (the rule of S, the offsets), tests/warp_area_ref.py (the rule on each axis) and tests/paste_nv12_ref.py /
tests/warp_paste_nv12_ref.py (the blend, the block rule).  float32 positions with every operation rounded, int64 everywhere else.  It knows
no culling, no tiles and no ownership: every row is evaluated over the WHOLE frame, one row after the other.

  counts(p, triangles, mats, W, H, mode, max_samples, min_scale)   T x 2 int32: (Sx, Sy) of every triangle of one row on a W x H frame
  sample(p, triangles, mats, lab, x, alpha, H, W, cnt, ...)        (q B, G, R, a, the triangle map, the footprint, the pixels with a
                                                                   refused sub-sample, the pixels with a sub-sample tap on label 255)
  paste_row(pix, fmt, ...) / paste_row_nv12(Y, UV, ...)            one row in place; what sample() returns (NV12: and the chroma written)
"""
import numpy as np

import align_area_ref as AR
import align_tensor_ref as T
import paste_nv12_ref as N
import paste_ref as P
import warp_area_ref as WA
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as R

f32 = np.float32
BILINEAR, AREA = AR.BILINEAR, AR.AREA


def counts(p, triangles, mats, W, H, mode=AREA, max_samples=16, min_scale=1.0):
    """item 2: the rule of S on (W00^2 + W10^2, W01^2 + W11^2) of the float32 W_t; (1, 1) for a DEGENERATE row, a row whose box is empty
    and a triangle that is skipped (d == 0, an entry of W_t not finite) or covers nothing (det E == 0)"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = np.ones((tri.shape[0], 2), np.int32)
    if not np.isfinite(np.asarray(p, f32)).all() or WP.box(p, W, H) == (0, 0, 0, 0):
        return out
    Wt, skipped = WP.inverses(mats)
    det = WP.det_e(p, tri)
    s = WA.samples(Wt, False, mode, max_samples, min_scale)
    live = ~skipped & (det != 0)
    out[live] = s[live]
    return out


def _taps(px, amap, u, v):
    """the unrounded sums of the four taps at float32 positions (any shape): (q shape + (C,), a shape, accepted, a tap on amap < 0)"""
    ch, cw = px.shape[:2]
    with np.errstate(all="ignore"):
        ok = T.accepted(u, v)
        U = np.floor(np.where(ok, u, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
        V = np.floor(np.where(ok, v, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
    u0, fu, v0, fv = U >> 5, U & 31, V >> 5, V & 31
    q, a = np.zeros(u.shape + (px.shape[2],), np.int64), np.zeros(u.shape, np.int64)
    hull = np.zeros(u.shape, bool)
    for dx, dy, wt in ((0, 0, (32 - fu) * (32 - fv)), (1, 0, fu * (32 - fv)), (0, 1, (32 - fu) * fv), (1, 1, fu * fv)):
        xx, yy = u0 + dx, v0 + dy
        inside = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        xc, yc = np.clip(xx, 0, cw - 1), np.clip(yy, 0, ch - 1)
        q += wt[..., None] * px[yc, xc]
        a += wt * np.where(inside, np.maximum(amap[yc, xc], 0), 0)
        hull |= inside & (amap[yc, xc] < 0) & (wt > 0) & ok
    return q, a, ok, hull


def sample(p, triangles, mats, lab, x, alpha, H, Wd, cnt, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0),
           gray_shift=14, origin=(0, 0)):
    """Items 1, 3 and 4 for one row over the H x W window of the frame that starts at ``origin``: the unfiltered footprint from the pixel
    centres; per triangle the Sx x Sy sub-samples through its own W_t, averaged.  a is 0 outside the footprint."""
    cnt = np.asarray(cnt).reshape(-1, 2)
    tmap = WP.triangle_map(p, triangles, mats, Wd, H, origin=origin)
    Wt, _ = WP.inverses(mats)
    px = P.decode(P.as_hwc(x, layout, channels), scale, bias)              # ch x cw x C
    ch, cw = px.shape[:2]
    amap = np.full((ch, cw), 255, np.int64) if alpha is None else np.asarray(alpha, np.uint8).astype(np.int64)
    amap = np.where(np.asarray(lab) == R.NONE, -1, amap)                   # (-1: label 255, read as 0 and counted)
    has = tmap >= 0
    w = Wt[np.where(has, tmap, 0)]
    X = np.broadcast_to(np.arange(origin[0], origin[0] + Wd, dtype=f32)[None, :], (H, Wd))
    Y = np.broadcast_to(np.arange(origin[1], origin[1] + H, dtype=f32)[:, None], (H, Wd))
    with np.errstate(all="ignore"):
        u = ((w[..., 0] * X + w[..., 1] * Y).astype(f32) + w[..., 2]).astype(f32)
        v = ((w[..., 3] * X + w[..., 4] * Y).astype(f32) + w[..., 5]).astype(f32)
    q1, a1, ok, hull1 = _taps(px, amap, u, v)
    with np.errstate(all="ignore"):
        U = np.floor(np.where(ok, u, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
        V = np.floor(np.where(ok, v, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
    foot = ok & has & ((U >> 5) >= -1) & ((U >> 5) <= cw - 1) & ((V >> 5) >= -1) & ((V >> 5) <= ch - 1)
    q, a = (q1 + 512) >> 10, np.where(foot, (a1 + 512) >> 10, 0)           # n = 1: the unfiltered paste
    refused, hull = np.zeros((H, Wd), bool), hull1 & foot
    for t in np.unique(tmap[foot]):
        Sx, Sy = int(cnt[t, 0]), int(cnt[t, 1])
        if Sx == 1 and Sy == 1:
            continue
        ii, jj = np.nonzero(foot & (tmap == t))
        m = Wt[t]
        ox, oy = AR.offsets(Sx), AR.offsets(Sy)
        fX = ((jj + origin[0]).astype(f32)[:, None, None] + ox[None, None, :]).astype(f32)
        fY = ((ii + origin[1]).astype(f32)[:, None, None] + oy[None, :, None]).astype(f32)
        with np.errstate(all="ignore"):
            su = (((m[0] * fX).astype(f32) + (m[1] * fY).astype(f32)).astype(f32) + m[2]).astype(f32)
            sv = (((m[3] * fX).astype(f32) + (m[4] * fY).astype(f32)).astype(f32) + m[5]).astype(f32)
        qs, as_, oks, hs = _taps(px, amap, su, sv)
        n = Sx * Sy
        qs, as_ = np.where(oks[..., None], qs, 0).sum((1, 2)), np.where(oks, as_, 0).sum((1, 2))
        assert max(qs.max(initial=0), as_.max(initial=0)) + 512 * n < 2 ** 26 + 2 ** 17
        whole = oks.all((1, 2))
        q[ii, jj] = (qs + 512 * n) // (1024 * n)
        a[ii, jj] = np.where(whole, (as_ + 512 * n) // (1024 * n), 0)
        refused[ii, jj] = ~whole
        hull[ii, jj] = hs.any((1, 2))
    if channels == 3 and order == "rgb":
        q = q[..., ::-1]
    return q, a, tmap, foot, refused, hull


def paste_row(pix, fmt, p, triangles, mats, lab, x, alpha=None, cnt=None, channels=3, gray_shift=14, origin=(0, 0), **spec):
    """one row into a frame of one of the five per-pixel formats (H x W x bytes, in place)"""
    H, Wd = pix.shape[:2]
    out = sample(p, triangles, mats, lab, x, alpha, H, Wd, cnt, channels=channels, gray_shift=gray_shift, origin=origin, **spec)
    WN.blend_bgr(pix, fmt, out[0], out[1], channels, gray_shift)
    return out


def paste_row_nv12(Y, UV, p, triangles, mats, lab, x, alpha=None, cnt=None, channels=3, origin=(0, 0), **spec):
    """one row into the planes in place: warp_paste_nv12_ref.paste_row's block rule on the averaged q and a; returns sample()'s tuple and
    the chroma samples written"""
    H, Wd = Y.shape
    assert origin[0] % 2 == 0 and origin[1] % 2 == 0
    out = sample(p, triangles, mats, lab, x, alpha, H, Wd, cnt, channels=channels, origin=origin, **spec)
    q, a = out[0], out[1]
    yq = N.luma_of(q) if channels == 3 else q[..., 0]
    old = Y.astype(np.int64)
    Y[...] = np.where(a > 0, N.blend(a, yq, old), old).astype(np.uint8)
    if channels != 3:
        return out + (np.zeros(((H + 1) // 2, (Wd + 1) // 2), bool),)
    A = N.blocks(a)
    cntb = N.blocks(np.ones((H, Wd), np.int64))
    m = (N.blocks(a[..., None] * q) + (A // 2)[..., None]) // np.maximum(A, 1)[..., None]
    uq, vq = N.chroma_of(m)
    ac = (A + cntb // 2) // cntb
    old = UV.astype(np.int64)
    new = np.stack([N.blend(ac, uq, old[..., 0]), N.blend(ac, vq, old[..., 1])], -1)
    written = (A > 0) & (ac > 0)
    UV[...] = np.where(written[..., None], new, old).astype(np.uint8)
    return out + (written,)
