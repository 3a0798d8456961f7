"""The landmark region masks restated in numpy from the text of include/sdm.h ("Landmark region masks"): the vertices through the
float32 W, the convex hull (sort, exact turn, monotone chain), the signed distance with the non-zero winding rule, the map's byte.
Every float operation is one float32 numpy operation -- numpy rounds each on its own, and its float32 division and square root are
correctly rounded.  A plain module, imported like paste_ref."""
import numpy as np

import align_ref as A

f32 = np.float32
NONFINITE = 16
MAX_POS = f32(2.0 ** 20)


def inverse(M):
    """(W six float32, unusable): the inverse of the float32 M in float64, each entry rounded once"""
    m = np.asarray(M, f32).reshape(6).astype(np.float64)
    with np.errstate(all="ignore"):
        d = m[0] * m[4] - m[1] * m[3]
        w00, w01, w10, w11 = m[4] / d, -m[1] / d, -m[3] / d, m[0] / d
        w02, w12 = -(w00 * m[2] + w01 * m[5]), -(w10 * m[2] + w11 * m[5])
        W = np.array([w00, w01, w02, w10, w11, w12]).astype(f32)
    return W, bool(not np.isfinite(m).all() or d == 0 or not np.isfinite(W).all())


def vertices(W, points):
    """q (P x 2 float32) of the frame points (P x 2) through W"""
    W = np.asarray(W, f32)
    p = np.asarray(points, f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        qx = (W[0] * p[:, 0] + W[1] * p[:, 1]) + W[2]
        qy = (W[3] * p[:, 0] + W[4] * p[:, 1]) + W[5]
    return np.stack([qx, qy], 1)


def turn(o, a, b):
    d = [f32(a[0] - o[0]), f32(b[1] - o[1]), f32(a[1] - o[1]), f32(b[0] - o[0])]
    l, r = float(d[0]) * float(d[1]), float(d[2]) * float(d[3])          # exact: 24-bit factors in a 53-bit product
    return (l > r) - (l < r)


def hull(q):
    """the hull's vertices of the points q (m x 2 float32): lower chain, then upper chain"""
    pts = sorted({(float(x), float(y)) for x, y in np.asarray(q, f32)})
    if len(pts) == 1:
        return np.array(pts, f32)
    H = []
    for p in pts:
        while len(H) >= 2 and turn(H[-2], H[-1], p) <= 0:
            H.pop()
        H.append(p)
    t = len(H) + 1
    for p in pts[-2::-1]:
        while len(H) >= t and turn(H[-2], H[-1], p) <= 0:
            H.pop()
        H.append(p)
    return np.array(H[:-1], f32)


def signed_distance(q, width, height):
    """height x width float32: sd of every crop pixel to the polygon q (m x 2 float32, m >= 1)"""
    q = np.asarray(q, f32).reshape(-1, 2)
    Px, Py = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    D2 = np.full((height, width), np.inf, f32)
    wn = np.zeros((height, width), np.int32)
    zero, one = f32(0), f32(1)
    with np.errstate(all="ignore"):
        for k in range(len(q)):
            (ax, ay), (bx, by) = q[k], q[(k + 1) % len(q)]
            ex, ey = f32(bx - ax), f32(by - ay)
            wx, wy = Px - ax, Py - ay
            ee = f32(f32(ex * ex) + f32(ey * ey))
            t = np.minimum(np.maximum(((wx * ex) + (wy * ey)) / ee, zero), one) if ee > 0 else np.zeros_like(Px)
            dx, dy = wx - (t * ex), wy - (t * ey)
            D2 = np.minimum(D2, (dx * dx) + (dy * dy))
            cr = (ex * wy) - (ey * wx)
            wn += ((ay <= Py) & (by > Py) & (cr > 0)).astype(np.int32)
            wn -= (~(ay <= Py) & (by <= Py) & (cr < 0)).astype(np.int32)
    assert D2.dtype == f32
    sd = np.sqrt(D2)
    return np.where(wn != 0, -sd, sd).astype(f32)


def polygons_of(q, sizes, hull_bits):
    """the vertex lists of one row: q (P x 2) cut by sizes, polygon g replaced by its hull where bit g is set"""
    out, at = [], 0
    for g, m in enumerate(sizes):
        out.append(hull(q[at:at + m]) if hull_bits >> g & 1 else np.asarray(q[at:at + m], f32))
        at += m
    return out


def distance_map(polys, n_holes, width, height):
    """s, height x width float32, of one row's vertex lists (the last n_holes are holes)"""
    s = np.full((height, width), np.inf, f32)
    for g, q in enumerate(polys):
        sd = signed_distance(q, width, height)
        s = np.maximum(s, -sd) if g >= len(polys) - n_holes else np.minimum(s, sd)
    return s


def bytes_of(s, grow=0.0, feather=0.0):
    """the map's bytes of s (None: a flagged row, zeros are the caller's)"""
    wr = max(f32(feather), f32(1))
    a = f32(0.5) + ((f32(grow) - s) / wr)
    assert a.dtype == f32
    return np.rint(np.minimum(np.maximum(a, f32(0)), f32(1)) * f32(255)).astype(np.uint8)


def rasterise(polys, n_holes, width, height, grow=0.0, feather=0.0):
    return bytes_of(distance_map(polys, n_holes, width, height), grow, feather)


def mask_row(M, points, sizes, n_holes=0, hull_bits=0, width=16, height=16, grow=0.0, feather=0.0, flags_in=0):
    """(map height x width uint8, flags, vertex lists or None) of one row: M crop -> frame (6 float32), points P x 2 in the frame.
    flags_in: the fit's flags (the _at form: 0)"""
    s, flags, polys = row_state(M, points, sizes, n_holes, hull_bits, width, height, flags_in)
    return (np.zeros((height, width), np.uint8) if s is None else bytes_of(s, grow, feather)), flags, polys


def row_state(M, points, sizes, n_holes=0, hull_bits=0, width=16, height=16, flags_in=0):
    """(s height x width float32 or None for a flagged row, flags, vertex lists or None): everything of a row but grow and feather"""
    M = np.asarray(M, f32).reshape(6)
    W, bad = inverse(M)
    if not np.isfinite(M).all():
        return None, A.DEGENERATE, None
    if bad or flags_in & A.DEGENERATE:
        return None, flags_in | A.DEGENERATE, None
    q = vertices(W, points)
    if not (np.abs(q) <= MAX_POS).all():                                 # (false for a NaN)
        return None, flags_in | NONFINITE, None
    polys = polygons_of(q, sizes, hull_bits)
    return distance_map(polys, n_holes, width, height), flags_in, polys


def masks(mats, points, sizes, n_holes=0, hull_bits=0, width=16, height=16, grow=0.0, feather=0.0, flags_in=None):
    """(N x height x width uint8, flags N int32) of N rows"""
    out = [mask_row(m, p, sizes, n_holes, hull_bits, width, height, grow, feather, 0 if flags_in is None else int(flags_in[n]))
           for n, (m, p) in enumerate(zip(np.asarray(mats, f32).reshape(-1, 6), np.asarray(points, f32)))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)
