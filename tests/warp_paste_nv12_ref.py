"""Host restatement of the piecewise-affine paste into NV12 frames (include/sdm.h, "Pasting warped faces back into NV12 frames") in
numpy: the composition of the two restatements the suite already trusts.  sample() is the sampling half of
tests/warp_paste_ref.py's paste_row -- the triangle map, the per-triangle W_t, opacity 0 on label 255 --, and the block rule is built
from tests/paste_nv12_ref.py's blend, luma_of, chroma_of and blocks.  It knows no box culling, no tiles and no ownership: every row is
evaluated over the WHOLE frame, one row after the other, each reading the luma and the chroma the previous one left.

  sample(p, triangles, mats, lab, x, alpha, H, W, ...)   (q H x W x 3 int64 as B, G, R -- H x W x 1 for a 1-channel tensor --, a H x W
                                                         int64, the triangle map, the footprint): what the blend takes, before the blend
  paste_row(Y, UV, p, triangles, mats, lab, x, alpha, ...)   one row into the planes in place; returns (a, triangle map, footprint,
                                                         the chroma samples written)
  paste(Y, UV, rows, triangles, lab, **spec)             rows = [(p, mats, x, alpha), ...] in row order
"""
import numpy as np

import align_tensor_ref as T
import paste_nv12_ref as N
import paste_ref as P
import warp_paste_ref as WP
import warp_ref as R

f32 = np.float32


def sample(p, triangles, mats, lab, x, alpha, H, Wd, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0), gray_shift=14,
           origin=(0, 0)):
    """The colour and the opacity of one mesh row at every pixel of the H x W window of the frame that starts at ``origin``: the
    formulas of "Pasting warped faces back".  a is 0 outside the row's footprint."""
    tmap = WP.triangle_map(p, triangles, mats, Wd, H, origin=origin)
    Wt, _ = WP.inverses(mats)
    px = P.decode(P.as_hwc(x, layout, channels), scale, bias)              # ch x cw x C
    ch, cw = px.shape[:2]
    has = tmap >= 0
    w = Wt[np.where(has, tmap, 0)]                                         # H x W x 6 float32
    X = np.broadcast_to(np.arange(origin[0], origin[0] + Wd, dtype=f32)[None, :], (H, Wd))
    Y = np.broadcast_to(np.arange(origin[1], origin[1] + H, dtype=f32)[:, None], (H, Wd))
    with np.errstate(all="ignore"):
        u = ((w[..., 0] * X + w[..., 1] * Y).astype(f32) + w[..., 2]).astype(f32)
        v = ((w[..., 3] * X + w[..., 4] * Y).astype(f32) + w[..., 5]).astype(f32)
        ok = T.accepted(u, v) & has
        U = np.floor(np.where(ok, u, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
        V = np.floor(np.where(ok, v, f32(0)) * f32(32) + f32(0.5)).astype(np.int64)
    u0, fu, v0, fv = U >> 5, U & 31, V >> 5, V & 31
    foot = ok & (u0 >= -1) & (u0 <= cw - 1) & (v0 >= -1) & (v0 <= ch - 1)
    amap = np.full((ch, cw), 255, np.int64) if alpha is None else np.asarray(alpha, np.uint8).astype(np.int64)
    amap = np.where(np.asarray(lab) == R.NONE, 0, amap)                    # a tap on an unlabelled crop pixel reads 0
    q, a = np.zeros((H, Wd, px.shape[2]), np.int64), np.zeros((H, Wd), np.int64)
    for dx, dy, wt in ((0, 0, (32 - fu) * (32 - fv)), (1, 0, fu * (32 - fv)), (0, 1, (32 - fu) * fv), (1, 1, fu * fv)):
        xx, yy = u0 + dx, v0 + dy
        inside = (xx >= 0) & (xx < cw) & (yy >= 0) & (yy < ch)
        xc, yc = np.clip(xx, 0, cw - 1), np.clip(yy, 0, ch - 1)
        q += wt[..., None] * px[yc, xc]
        a += wt * np.where(inside, amap[yc, xc], 0)
    q, a = (q + 512) >> 10, np.where(foot, (a + 512) >> 10, 0)
    if channels == 3 and order == "rgb":
        q = q[..., ::-1]
    return q, a, tmap, foot


def blend_bgr(pix, fmt, q, a, channels=3, gray_shift=14):
    """q and a of sample() blended into a frame of one of the five per-pixel formats (H x W x bytes, in place): what
    warp_paste_ref.paste_row does behind its own sampling"""
    bgr = q if channels == 3 else np.repeat(q, 3, -1)
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
    pix[..., :nb] = np.where((a > 0)[..., None], N.blend(a[..., None], val, old), old).astype(np.uint8)


def paste_row(Y, UV, p, triangles, mats, lab, x, alpha=None, channels=3, origin=(0, 0), **spec):
    """one row into the planes in place (Y: H x W uint8, UV: ceil(H/2) x ceil(W/2) x 2 uint8); returns (a, triangle map, footprint, the
    chroma samples written: ceil(H/2) x ceil(W/2) bool).  origin =
    (X0, Y0), both EVEN, as for paste_nv12_ref.paste_row: a window of odd width or height must end at the frame's own odd edge"""
    H, Wd = Y.shape
    assert origin[0] % 2 == 0 and origin[1] % 2 == 0
    q, a, tmap, foot = sample(p, triangles, mats, lab, x, alpha, H, Wd, channels=channels, origin=origin, **spec)
    yq = N.luma_of(q) if channels == 3 else q[..., 0]
    old = Y.astype(np.int64)
    Y[...] = np.where(a > 0, N.blend(a, yq, old), old).astype(np.uint8)
    if channels != 3:
        return a, tmap, foot, np.zeros(((H + 1) // 2, (Wd + 1) // 2), bool)   # the UV plane is neither read nor written
    A = N.blocks(a)                                                        # (a pixel outside the hull or the box: a_i = 0)
    cnt = N.blocks(np.ones((H, Wd), np.int64))                             # (... and it still counts here)
    m = (N.blocks(a[..., None] * q) + (A // 2)[..., None]) // np.maximum(A, 1)[..., None]
    uq, vq = N.chroma_of(m)
    ac = (A + cnt // 2) // cnt
    old = UV.astype(np.int64)
    new = np.stack([N.blend(ac, uq, old[..., 0]), N.blend(ac, vq, old[..., 1])], -1)
    written = (A > 0) & (ac > 0)
    UV[...] = np.where(written[..., None], new, old).astype(np.uint8)
    return a, tmap, foot, written


def paste(Y, UV, rows, triangles, lab, **spec):
    """rows: (p K x 2, mats T x 6, x, alpha) in row order, each reading what the previous one left"""
    return [paste_row(Y, UV, p, triangles, m, lab, x, alpha, **spec) for p, m, x, alpha in rows]
