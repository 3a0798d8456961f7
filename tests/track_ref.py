"""Host restatement of the tracker's two rules (include/sdm.h, sdm_track_*; csrc/sdm_track.hip), in the device's float32 arithmetic
(every operation rounded, nothing contracted), and straightforward float64 versions to check it against.

  realign(prev, mean)            the mean placed in the enclosing box of a landmark row
  lost_mask(init, res, W, H, ...) the lost decision of a result row: SDM_TRACK_LOST_* bits, 0 = tracked
"""
import numpy as np

NONFINITE, SMALL, OUTSIDE, SCALE = 1, 2, 4, 8
f32 = np.float32


def _bounds(rows):
    rows = np.atleast_2d(rows)
    L = rows.shape[1] // 2
    return rows[:, :L].min(1), rows[:, :L].max(1), rows[:, L:].min(1), rows[:, L:].max(1)


def realign(prev, mean):
    """x0[j] = ((m[j] - mx0) / (mx1 - mx0)) * (bx1 - bx0) + bx0 (y likewise), float32, one rounding per operation."""
    prev = np.atleast_2d(np.asarray(prev, f32))
    m = np.asarray(mean, f32).reshape(-1)
    L = m.size // 2
    bx0, bx1, by0, by1 = (v[:, None] for v in _bounds(prev))
    mx0, mx1, my0, my1 = m[:L].min(), m[:L].max(), m[L:].min(), m[L:].max()
    out = np.empty_like(prev)
    out[:, :L] = ((m[:L] - mx0) / (mx1 - mx0)) * (bx1 - bx0) + bx0
    out[:, L:] = ((m[L:] - my0) / (my1 - my0)) * (by1 - by0) + by0
    return out


def realign64(prev, mean):
    prev = np.atleast_2d(np.asarray(prev, np.float64))
    m = np.asarray(mean, np.float64).reshape(-1)
    L = m.size // 2
    out = np.empty_like(prev)
    for r in range(prev.shape[0]):
        for lo, hi in ((0, L), (L, 2 * L)):
            b, mm = prev[r, lo:hi], m[lo:hi]
            out[r, lo:hi] = (mm - mm.min()) / (mm.max() - mm.min()) * (b.max() - b.min()) + b.min()
    return out


def ied(rows, right_eye, left_eye):
    """get_ied (include/rcr/helpers.hpp:136-160) as the device evaluates it: float32 eye centres (sums in index order, then a
    division), the distance in double."""
    rows = np.atleast_2d(np.asarray(rows, f32))
    L = rows.shape[1] // 2
    out = np.empty(rows.shape[0])
    for r in range(rows.shape[0]):
        c = []
        for eye in (right_eye, left_eye):
            sx, sy = f32(0), f32(0)
            for i in eye:
                sx, sy = f32(sx + rows[r, i]), f32(sy + rows[r, L + i])
            c.append((f32(sx / f32(len(eye))), f32(sy / f32(len(eye)))))
        dx, dy = float(f32(c[0][0] - c[1][0])), float(f32(c[0][1] - c[1][1]))
        out[r] = np.sqrt(dx * dx + dy * dy)
    return out


def lost_mask(init, res, width, height, min_size, max_scale_change=0.0, right_eye=(), left_eye=()):
    """Per row: NONFINITE alone when a coordinate of ``res`` is not finite, else SMALL | OUTSIDE | SCALE as include/sdm.h states
    them, in float32 (the box, its centre) and double (the inter-eye distances and their comparison).  width / height: of each
    row's image (scalars or one per row)."""
    res = np.atleast_2d(np.asarray(res, f32))
    n = res.shape[0]
    W = np.broadcast_to(np.asarray(width), (n,))
    H = np.broadcast_to(np.asarray(height), (n,))
    out = np.zeros(n, np.int32)
    finite = np.isfinite(res).all(1)
    bx0, bx1, by0, by1 = _bounds(np.where(finite[:, None], res, f32(0)))
    use_scale = len(right_eye) > 0 and len(left_eye) > 0 and max_scale_change > 0
    if use_scale:
        ir, ii, k = ied(res, right_eye, left_eye), ied(init, right_eye, left_eye), float(f32(max_scale_change))
    for r in range(n):
        if not finite[r]:
            out[r] = NONFINITE
            continue
        m = 0
        if f32(bx1[r] - bx0[r]) < f32(min_size) or f32(by1[r] - by0[r]) < f32(min_size):
            m |= SMALL
        cx, cy = f32(f32(bx0[r] + bx1[r]) * f32(0.5)), f32(f32(by0[r] + by1[r]) * f32(0.5))
        if not (cx >= 0 and cx < f32(W[r]) and cy >= 0 and cy < f32(H[r])):
            m |= OUTSIDE
        if use_scale and (ir[r] > ii[r] * k or ir[r] * k < ii[r]):
            m |= SCALE
        out[r] = m
    return out


def lost_mask64(init, res, width, height, min_size, max_scale_change=0.0, right_eye=(), left_eye=()):
    """The same rule written plainly in float64 (agrees with ``lost_mask`` away from the thresholds)."""
    res = np.atleast_2d(np.asarray(res, np.float64))
    init = np.atleast_2d(np.asarray(init, np.float64))
    L = res.shape[1] // 2
    n = res.shape[0]
    W = np.broadcast_to(np.asarray(width, np.float64), (n,))
    H = np.broadcast_to(np.asarray(height, np.float64), (n,))

    def ied64(row):
        r = np.array([row[list(right_eye)].mean(), row[[L + i for i in right_eye]].mean()])
        l = np.array([row[list(left_eye)].mean(), row[[L + i for i in left_eye]].mean()])
        return np.linalg.norm(r - l)

    out = np.zeros(n, np.int32)
    for i in range(n):
        x, y = res[i, :L], res[i, L:]
        if not np.isfinite(res[i]).all():
            out[i] = NONFINITE
            continue
        m = 0
        if x.max() - x.min() < min_size or y.max() - y.min() < min_size:
            m |= SMALL
        cx, cy = (x.min() + x.max()) / 2, (y.min() + y.max()) / 2
        if not (0 <= cx < W[i] and 0 <= cy < H[i]):
            m |= OUTSIDE
        if len(right_eye) and len(left_eye) and max_scale_change > 0:
            a, b = ied64(res[i]), ied64(init[i])
            if a > b * max_scale_change or a * max_scale_change < b:
                m |= SCALE
        out[i] = m
    return out
