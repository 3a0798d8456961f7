"""Host restatement of the piecewise-affine face warp (include/sdm.h, "Warped faces"; csrc/sdm_capi_warp.hip, csrc/sdm_warp.hip): the
label map, the triangles' constants and the per-row matrices in float64 with the header's operation order (numpy rounds every operation
and contracts nothing), the flags, and the pixels through the functions of tests/align_ref.py and tests/align_tensor_ref.py at the
positions each pixel's own triangle gives.

  constants(template, triangles)                  (G T x 2 x 2, q_a T x 2, D T) float64
  labels(template, triangles, width, height)      height x width uint8, 255 = no triangle
  matrices(rows, landmark_index, template, triangles)   N x T x 6 float32 (NaN rows where degenerate)
  flags(rows, landmark_index, template, triangles, sizes)   N int, sizes: (W, H) of every row's image
  warped(frame, mats, lab)                        (kind, (B, G, R) int64 height x width x 3, luma or None) of one row
  tensor(frame, mats, lab, **spec)                the crop in its layout
"""
import numpy as np

import align_ref as A
import align_tensor_ref as T

DEGENERATE, PARTIAL, FOLDED = 1, 2, 4
NONE = 255
f32, f64 = np.float32, np.float64


def _pts(template):
    return np.asarray(template, f32).astype(f64).reshape(-1, 2)


def constants(template, triangles):
    q = _pts(template)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    qa, qb, qc = q[tri[:, 0]], q[tri[:, 1]], q[tri[:, 2]]
    u, v = qb - qa, qc - qa
    D = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    G = np.stack([np.stack([v[:, 1] / D, -v[:, 0] / D], -1), np.stack([-u[:, 1] / D, u[:, 0] / D], -1)], 1)
    return G, qa, D


def edge_functions(template, triangles, width, height):
    """T x 3 x height x width float64: e0, e1, e2 of every triangle (b and c exchanged where D < 0) at every pixel centre"""
    q = _pts(template)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3).copy()
    _, _, D = constants(template, triangles)
    swap = D < 0
    tri[swap, 1], tri[swap, 2] = tri[swap, 2].copy(), tri[swap, 1].copy()
    x = np.arange(width, dtype=f64)[None, None, :]
    y = np.arange(height, dtype=f64)[None, :, None]
    out = []
    for p, r in ((0, 1), (1, 2), (2, 0)):
        P, R = q[tri[:, p]][:, :, None, None], q[tri[:, r]][:, :, None, None]
        out.append((R[:, 0] - P[:, 0]) * (y - P[:, 1]) - (R[:, 1] - P[:, 1]) * (x - P[:, 0]))
    return np.stack(out, 1)


def labels(template, triangles, width, height):
    e = edge_functions(template, triangles, width, height)
    inside = (e >= 0).all(1)                                  # T x height x width
    first = inside.argmax(0)
    return np.where(inside.any(0), first, NONE).astype(np.uint8)


def _landmarks(rows, landmark_index):
    rows = np.atleast_2d(np.asarray(rows, f32))
    L = rows.shape[1] // 2
    idx = np.asarray(landmark_index, np.int64)
    return np.stack([rows[:, idx], rows[:, L + idx]], -1)     # N x K x 2 float32


def degenerate(rows, landmark_index):
    return ~np.isfinite(_landmarks(rows, landmark_index)).all((1, 2))


def _fit(rows, landmark_index, template, triangles):
    p = _landmarks(rows, landmark_index).astype(f64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    G, qa, D = constants(template, triangles)
    pa, pb, pc = p[:, tri[:, 0]], p[:, tri[:, 1]], p[:, tri[:, 2]]          # N x T x 2
    with np.errstate(invalid="ignore", over="ignore"):
        e0, e1 = pb - pa, pc - pa                                            # columns of E: E_r0 = e0[..., r], E_r1 = e1[..., r]
        lin = np.empty(p.shape[:1] + (tri.shape[0], 2, 2))
        for r in range(2):
            for c in range(2):
                lin[:, :, r, c] = e0[..., r] * G[None, :, 0, c] + e1[..., r] * G[None, :, 1, c]
        t = np.stack([pa[..., r] - (lin[:, :, r, 0] * qa[None, :, 0] + lin[:, :, r, 1] * qa[None, :, 1]) for r in range(2)], -1)
        det = e0[..., 0] * e1[..., 1] - e1[..., 0] * e0[..., 1]
    return lin, t, det, D


def matrices(rows, landmark_index, template, triangles):
    lin, t, _, _ = _fit(rows, landmark_index, template, triangles)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.concatenate([lin, t[..., None]], -1).reshape(lin.shape[0], lin.shape[1], 6).astype(f32)
    m[degenerate(rows, landmark_index)] = np.nan
    return m


def flags(rows, landmark_index, template, triangles, sizes):
    p = _landmarks(rows, landmark_index)
    _, _, det, D = _fit(rows, landmark_index, template, triangles)
    out = np.zeros(p.shape[0], np.int32)
    for n, (W, H) in enumerate(sizes):
        if not np.isfinite(p[n]).all():
            out[n] = DEGENERATE
            continue
        inside = (p[n, :, 0] >= 0) & (p[n, :, 0] <= f32(W - 1)) & (p[n, :, 1] >= 0) & (p[n, :, 1] <= f32(H - 1))
        if not inside.all():
            out[n] |= PARTIAL
        if not (((det[n] > 0) & (D > 0)) | ((det[n] < 0) & (D < 0))).all():
            out[n] |= FOLDED
    return out


def positions(mats, lab):
    """float32 source positions of every crop pixel through its own triangle's matrix; NaN where there is no triangle"""
    h, w = lab.shape
    sx, sy = np.full((h, w), np.nan, f32), np.full((h, w), np.nan, f32)
    for t in np.unique(lab):
        if t == NONE:
            continue
        tx, ty = A.positions(np.asarray(mats, f32)[t], w, h)
        sx[lab == t], sy[lab == t] = tx[lab == t], ty[lab == t]
    return sx, sy


def warped(frame, mats, lab):
    """one row: (kind, (B, G, R) int64 height x width x 3, the luma warp of an NV12 frame or None); 0 where there is no triangle"""
    sx, sy = positions(mats, lab)
    if frame.fmt == T.GRAY:
        g = T.warp_at(frame.pix[..., None], sx, sy, 0)
        return "gray", np.repeat(g, 3, -1), None
    if frame.fmt in (T.BGR, T.RGB, T.BGRA, T.RGBA):
        v = T.warp_at(frame.pix, sx, sy, 0)[..., :3]
        return "colour", (v[..., ::-1] if frame.fmt in (T.RGB, T.RGBA) else v), None
    y = T.warp_at(frame.pix[..., None], sx, sy, 0)
    ok = T.accepted(sx, sy)
    with np.errstate(invalid="ignore"):
        cx, cy = (sx * f32(0.5)).astype(f32), (sy * f32(0.5)).astype(f32)
    uv = T.warp_at(frame.uv, cx, cy, 128)
    bgr = T.nv12_to_bgr(y[..., 0], uv[..., 0], uv[..., 1])
    return "nv12", np.where(ok[..., None], bgr, 0), y[..., 0]


def tensor(frame, mats, lab, **spec):
    kind, bgr, y = warped(frame, mats, lab)
    return T.finish(kind, bgr, y, **spec)
