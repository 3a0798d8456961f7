"""Host restatement of the piecewise-affine paste (include/sdm.h, "Pasting warped faces back"; csrc/sdm_warp_paste_device.h) in numpy:
float64 on the float32 landmarks where the header says double, float32 positions, every operation rounded, int64 everywhere else.  It
knows no box culling, no tile culling and no ownership: every row is pasted over the WHOLE frame, every triangle is tested for every
pixel, one row after the other.  The row's box and every triangle's box are rules of the contract (a pixel outside is not covered) and
are restated as such: as comparisons in float64 on whole-frame arrays, not as loop bounds.

  points_of(rows, landmark_index)                 N x K x 2 float32: the mesh landmarks of N x 2L rows
  matrices(points, template, triangles)           N x T x 6 float32 A_t (tests/warp_ref.py on the points)
  flags(points, template, triangles, sizes)       N int, sizes: (W, H) of every row's destination frame
  box(p, W, H)                                    (x0, y0, x1, y1) of one row's K x 2 points, all 0 for an empty or degenerate one
  inverses(mats)                                  (W_t T x 6 float32, skipped T bool) of one row's T x 6 matrices
  triangle_map(p, triangles, mats, W, H)          H x W int64: the triangle of every frame pixel, -1 = none (the box applied)
  paste_row(pix, fmt, p, triangles, mats, lab, x, alpha, ...)   one row into pix in place; returns (footprint, opacity, triangle map)
  paste(pix, fmt, rows, triangles, lab, ...)      rows = [(p, mats, x, alpha), ...] in row order
"""
import numpy as np

import align_tensor_ref as T
import paste_ref as P
import warp_ref as R

f32, f64 = np.float32, np.float64
DEGENERATE, PARTIAL, FOLDED = R.DEGENERATE, R.PARTIAL, R.FOLDED


def points_of(rows, landmark_index):
    return R._landmarks(rows, landmark_index)


def _as_rows(points):
    """N x K x 2 points as N x 2K rows whose landmark k is column k: what tests/warp_ref.py reads"""
    p = np.asarray(points, f32)
    p = p[None] if p.ndim == 2 else p
    return np.concatenate([p[..., 0], p[..., 1]], 1), np.arange(p.shape[1])


def matrices(points, template, triangles):
    rows, idx = _as_rows(points)
    return R.matrices(rows, idx, template, triangles).reshape(rows.shape[0], -1, 6)


def flags(points, template, triangles, sizes):
    rows, idx = _as_rows(points)
    return R.flags(rows, idx, template, triangles, sizes)


def _clip(lo, hi, n):
    """[lo, hi) in float64, clipped to [0, n) before the conversion to int"""
    return int(min(max(lo, 0.0), float(n))), int(max(min(hi, float(n)), 0.0))


def box(p, W, H):
    p = np.asarray(p, f32)
    if not np.isfinite(p).all():
        return 0, 0, 0, 0
    d = p.astype(f64)
    x0, x1 = _clip(np.floor(d[:, 0].min()), np.ceil(d[:, 0].max()) + 1.0, W)
    y0, y1 = _clip(np.floor(d[:, 1].min()), np.ceil(d[:, 1].max()) + 1.0, H)
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)


def inverses(mats):
    m = np.asarray(mats, f32).reshape(-1, 6)
    inv = [P.inverse(a) for a in m]
    return np.stack([w for w, _ in inv]), np.array([bad for _, bad in inv], bool)


def det_e(p, triangles):
    """T float64: E00 E11 - E01 E10 of every triangle (the FOLDED rule's expression)"""
    d = np.asarray(p, f32).astype(f64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    pa, pb, pc = d[tri[:, 0]], d[tri[:, 1]], d[tri[:, 2]]
    with np.errstate(all="ignore"):
        e0, e1 = pb - pa, pc - pa
        return e0[:, 0] * e1[:, 1] - e1[:, 0] * e0[:, 1]


def covers(p, t, tri, det, W, H, tri_box=True, origin=(0, 0)):
    """H x W bool: the pixel lies in the triangle's box -- floor(min) - 1 <= x < ceil(max) + 2 over its three corners, the same in y,
    in float64 -- and the three edge functions of triangle t (b and c exchanged where det E < 0) are >= 0 at the pixel centre"""
    d = np.asarray(p, f32).astype(f64)
    a, b, c = tri[t]
    if det[t] < 0:
        b, c = c, b
    x = np.arange(origin[0], origin[0] + W, dtype=f64)[None, :]
    y = np.arange(origin[1], origin[1] + H, dtype=f64)[:, None]
    cx, cy = d[[a, b, c], 0], d[[a, b, c], 1]
    ok = ((x >= np.floor(cx.min()) - 1.0) & (x < (np.ceil(cx.max()) + 1.0) + 1.0)
          & (y >= np.floor(cy.min()) - 1.0) & (y < (np.ceil(cy.max()) + 1.0) + 1.0))
    ok = ok if tri_box else np.ones((H, W), bool)                          # (tests only: what the edge functions alone would say)
    with np.errstate(all="ignore"):
        for q, r in ((d[a], d[b]), (d[b], d[c]), (d[c], d[a])):
            ok &= ((r[0] - q[0]) * (y - q[1]) - (r[1] - q[1]) * (x - q[0])) >= 0
    return ok


def triangle_map(p, triangles, mats, W, H, use_box=True, tri_box=True, origin=(0, 0)):
    """origin = (X0, Y0): the map of the W x H window of the frame that starts at frame pixel (X0, Y0); the window lies inside the frame,
    so the row's box clipped to the window's far corner and cut at its origin is the box clipped to the frame, seen from the window"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    out = np.full((H, W), -1, np.int64)
    if not np.isfinite(np.asarray(p, f32)).all():
        return out
    det = det_e(p, tri)
    _, skipped = inverses(mats)
    for t in range(tri.shape[0] - 1, -1, -1):                 # (descending: the lowest number is written last)
        if det[t] == 0 or skipped[t]:
            continue
        out[covers(p, t, tri, det, W, H, tri_box, origin)] = t
    if use_box:
        X0, Y0 = origin
        x0, y0, x1, y1 = box(p, X0 + W, Y0 + H)
        inside = np.zeros((H, W), bool)
        inside[max(y0 - Y0, 0):max(y1 - Y0, 0), max(x0 - X0, 0):max(x1 - X0, 0)] = True
        out[~inside] = -1
    return out


def paste_row(pix, fmt, p, triangles, mats, lab, x, alpha=None, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0),
              gray_shift=14, origin=(0, 0)):
    """origin = (X0, Y0): pix is the window of the frame that starts at frame pixel (X0, Y0), as for paste_ref.paste_row"""
    H, Wd = pix.shape[:2]
    tmap = triangle_map(p, triangles, mats, Wd, H, origin=origin)
    Wt, _ = inverses(mats)
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
    bgr = (q[..., ::-1] if order == "rgb" else q) if channels == 3 else np.repeat(q, 3, -1)
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
    return foot, a, tmap


def paste(pix, fmt, rows, triangles, lab, **spec):
    """rows: (p K x 2, mats T x 6, x, alpha) in row order, each reading what the previous one left"""
    return [paste_row(pix, fmt, p, triangles, m, lab, x, alpha, **spec) for p, m, x, alpha in rows]
