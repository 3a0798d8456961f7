"""Host restatement of the paste into NV12 frames (include/sdm.h, "Pasting crops back into NV12 frames") in numpy, on top of
tests/paste_ref.py (the inverse, the decode) and tests/paste_area_ref.py / tests/align_area_ref.py (S of a row, the offsets): float32
positions with every operation rounded, int64 everywhere else.  It knows no box, no footprint, no block ownership: every row is evaluated
over the WHOLE frame, one row after the other, each reading the luma and the chroma the previous one left.

  sample(M, x, alpha, S, H, W, ...)            (q H x W x 3 int64 as B, G, R -- H x W x 1 for a 1-channel tensor --, a H x W int64):
                                               what both paste restatements blend, before the blend
  paste_row(Y, UV, M, x, alpha, S, ...)        one row into the planes (Y: H x W uint8, UV: ceil(H/2) x ceil(W/2) x 2 uint8, in place)
  paste(Y, UV, rows, filter=None | (mode, max_samples, min_scale), **spec)      rows = [(M, x, alpha), ...]; returns [S, ...]
  bgr_of(Y, UV)                                the crop call's BT.601 decode of whole planes (align_tensor_ref's constants), for round trips
"""
import numpy as np

import align_area_ref as R
import align_tensor_ref as T
import paste_area_ref as Q
import paste_ref as P

f32 = np.float32


def sample(M, x, alpha, S, H, Wd, layout="nchw", channels=3, order="rgb", scale=(1, 1, 1), bias=(0, 0, 0), gray_shift=14, origin=(0, 0)):
    """The colour and the opacity of one non-degenerate row at every frame pixel: at S = 1 the formula of "Pasting crops back" (one
    sub-sample with offset 0: the same float32 expression), else the S x S average of "Pasting crops back, filtered"."""
    W, degenerate = P.inverse(M)
    assert not degenerate
    p = P.decode(P.as_hwc(x, layout, channels), scale, bias)                   # ch x cw x C
    ch, cw = p.shape[:2]
    o = R.offsets(S) if S > 1 else np.zeros(1, f32)
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
    q = (q.sum((2, 3)) + 512 * n) // (1024 * n)
    a = np.where(ok.all((2, 3)), (a.sum((2, 3)) + 512 * n) // (1024 * n), 0)
    if channels == 3 and order == "rgb":
        q = q[..., ::-1]
    return q, a


def blend(a, q, o):
    return (a * q + (255 - a) * o + 127) // 255


def luma_of(q):
    return (269484 * q[..., 2] + 528482 * q[..., 1] + 102760 * q[..., 0] + (16 << 20) + (1 << 19)) >> 20


def chroma_of(m):
    """(Uq, Vq) of a mean colour m (... x 3 as B, G, R)"""
    b, g, r = m[..., 0], m[..., 1], m[..., 2]
    uq = (460324 * b - 305135 * g - 155188 * r + (128 << 20) + (1 << 19)) >> 20
    vq = (460324 * r - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20
    return np.clip(uq, 0, 255), np.clip(vq, 0, 255)


def blocks(v):
    """the sums of v (H x W x ...) over the 2 x 2 blocks, a pixel outside the frame counting 0"""
    H, Wd = v.shape[:2]
    pad = np.zeros(((H + 1) // 2 * 2, (Wd + 1) // 2 * 2) + v.shape[2:], np.int64)
    pad[:H, :Wd] = v
    return pad.reshape((pad.shape[0] // 2, 2, pad.shape[1] // 2, 2) + v.shape[2:]).sum((1, 3))


def paste_row(Y, UV, M, x, alpha=None, S=1, channels=3, origin=(0, 0), **spec):
    """returns the row's opacity a (H x W); a degenerate row pastes nothing.  origin = (X0, Y0), both EVEN: Y and UV are the windows of
    the planes that start at luma pixel (X0, Y0) and chroma sample (X0 / 2, Y0 / 2); a window of odd width or height must end at the
    frame's own odd edge (a pixel beyond the window counts as outside the frame)"""
    H, Wd = Y.shape
    assert origin[0] % 2 == 0 and origin[1] % 2 == 0
    if P.inverse(M)[1]:
        return np.zeros((H, Wd), np.int64)
    q, a = sample(M, x, alpha, S, H, Wd, channels=channels, origin=origin, **spec)
    yq = luma_of(q) if channels == 3 else q[..., 0]
    old = Y.astype(np.int64)
    Y[...] = np.where(a > 0, blend(a, yq, old), old).astype(np.uint8)
    if channels != 3:
        return a                                                               # the UV plane is neither read nor written
    A = blocks(a)
    cnt = blocks(np.ones((H, Wd), np.int64))
    safe = np.maximum(A, 1)
    m = (blocks(a[..., None] * q) + (A // 2)[..., None]) // safe[..., None]
    uq, vq = chroma_of(m)
    ac = (A + cnt // 2) // cnt
    old = UV.astype(np.int64)
    new = np.stack([blend(ac, uq, old[..., 0]), blend(ac, vq, old[..., 1])], -1)
    UV[...] = np.where(((A > 0) & (ac > 0))[..., None], new, old).astype(np.uint8)
    return a


def paste(Y, UV, rows, filter=None, **spec):
    """rows: (M, x, alpha) in row order; filter: None (plain bilinear) or (mode, max_samples, min_scale); returns S of every row"""
    out = []
    for M, x, alpha in rows:
        S = 1 if filter is None or P.inverse(M)[1] else Q.samples(M, *filter)
        paste_row(Y, UV, M, x, alpha, S, **spec)
        out.append(S)
    return out


def bgr_of(Y, UV):
    """every pixel of an NV12 frame through the crop call's decode at its own chroma sample: H x W x 3 uint8 as B, G, R"""
    H, Wd = Y.shape
    uv = np.repeat(np.repeat(UV, 2, 0), 2, 1)[:H, :Wd].astype(np.int64)
    return T.nv12_to_bgr(Y.astype(np.int64), uv[..., 0], uv[..., 1])
