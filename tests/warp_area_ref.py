"""Host restatement of sdm_warp_crops_tensor_filtered (include/sdm.h, "Warped faces, filtered"; csrc/sdm_warp_area.hip) on top of
tests/warp_ref.py (labels, matrices) and tests/align_area_ref.py (the rule of S, the offsets, the un-rounded sub-sample value): (Sx, Sy) of
every triangle, the sub-samples of a pixel through its own triangle's matrix, the average over n = Sx Sy and the NV12 / channel rules on
the averaged values.  numpy float32 operations one at a time, integers in int64.  Nothing here calls the library.

  samples(mats, degenerate, mode, max_samples, min_scale)   T x 2 int32: (Sx, Sy) of every triangle of one row
  positions(m, jj, ii, Sx, Sy)                            float32 sx, sy of the sub-samples of the pixels (jj, ii): P x Sy (v) x Sx (u)
  warped(frame, mats, lab, samples)                       (kind, (B, G, R) int64 height x width x 3, averaged Y of an NV12 frame or None)
  tensor(frame, mats, lab, samples, **spec)               one crop in its layout, through align_tensor_ref.finish
"""
import numpy as np

import align_area_ref as AR
import align_tensor_ref as T
import warp_ref as R

BILINEAR, AREA = AR.BILINEAR, AR.AREA
f32 = np.float32


def squares(mats):
    """T x 2 float32: (cx2, cy2) = (A00 A00 + A10 A10, A01 A01 + A11 A11), every product and sum rounded"""
    m = np.asarray(mats, f32).reshape(-1, 6)
    with np.errstate(over="ignore", invalid="ignore"):
        cx2 = ((m[:, 0] * m[:, 0]).astype(f32) + (m[:, 3] * m[:, 3]).astype(f32)).astype(f32)
        cy2 = ((m[:, 1] * m[:, 1]).astype(f32) + (m[:, 4] * m[:, 4]).astype(f32)).astype(f32)
    return np.stack([cx2, cy2], -1)


def samples(mats, degenerate=False, mode=AREA, max_samples=AR.MAX_S, min_scale=1.0):
    """item 2: the rule of the rigid call's S on each of the two values"""
    return np.array([[AR.samples_of_s2(v, mode, max_samples, min_scale, degenerate) for v in pair] for pair in squares(mats)],
                    np.int32).reshape(-1, 2)


def positions(m, jj, ii, Sx, Sy):
    """item 3 for the pixels (column jj[p], row ii[p]) through the ONE matrix m"""
    m = np.asarray(m, f32).reshape(2, 3)
    ox, oy = AR.offsets(Sx), AR.offsets(Sy)
    fj = (np.asarray(jj).astype(f32)[:, None, None] + ox[None, None, :]).astype(f32)
    fi = (np.asarray(ii).astype(f32)[:, None, None] + oy[None, :, None]).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = ((m[0, 0] * fj).astype(f32) + (m[0, 1] * fi).astype(f32)).astype(f32) + m[0, 2]
        sy = ((m[1, 0] * fj).astype(f32) + (m[1, 1] * fi).astype(f32)).astype(f32) + m[1, 2]
    return sx.astype(f32), sy.astype(f32)


def average(q, n):
    """item 4: (sum over the n sub-samples + 512 n) // (1024 n); q: P x Sy x Sx x C"""
    total = q.sum((1, 2))
    assert total.max(initial=0) + 512 * n < 2 ** 26 + 2 ** 17
    return (total + 512 * n) // (1024 * n)


def warped(frame, mats, lab, samples):
    """one row: (kind, (B, G, R) int64 height x width x 3, y): warp_ref.warped with every pixel averaged over the Sx x Sy sub-samples its
    triangle asks for; 0 where there is no triangle or a sub-sample is refused; y: the averaged luma of an NV12 frame, None otherwise"""
    mats, samples = np.asarray(mats, f32).reshape(-1, 6), np.asarray(samples).reshape(-1, 2)
    h, w = lab.shape
    bgr, y = np.zeros((h, w, 3), np.int64), np.zeros((h, w), np.int64)
    kind = "gray" if frame.fmt == T.GRAY else "nv12" if frame.fmt == T.NV12 else "colour"
    for t in np.unique(lab):
        if t == R.NONE:
            continue
        ii, jj = np.nonzero(lab == t)
        Sx, Sy = int(samples[t, 0]), int(samples[t, 1])
        n = Sx * Sy
        sx, sy = positions(mats[t], jj, ii, Sx, Sy)
        whole = T.accepted(sx, sy).all((1, 2))[:, None]                     # a refused sub-sample zeroes the pixel
        if kind == "gray":
            bgr[ii, jj] = np.where(whole, average(AR.unrounded(frame.pix, sx, sy, 0), n), 0)
        elif kind == "colour":
            v = np.where(whole, average(AR.unrounded(frame.pix, sx, sy, 0), n), 0)[..., :3]       # alpha is never read
            bgr[ii, jj] = v[..., ::-1] if frame.fmt in (T.RGB, T.RGBA) else v
        else:
            lum = average(AR.unrounded(frame.pix, sx, sy, 0), n)
            with np.errstate(invalid="ignore"):
                cx, cy = (sx * f32(0.5)).astype(f32), (sy * f32(0.5)).astype(f32)
            uv = average(AR.unrounded(frame.uv, cx, cy, 128), n)
            bgr[ii, jj] = np.where(whole, T.nv12_to_bgr(lum[..., 0], uv[..., 0], uv[..., 1]), 0)
            y[ii, jj] = np.where(whole, lum, 0)[..., 0]
    return kind, bgr, (y if kind == "nv12" else None)


def tensor(frame, mats, lab, samples, **spec):
    kind, bgr, y = warped(frame, mats, lab, samples)
    return T.finish(kind, bgr, y, **spec)
