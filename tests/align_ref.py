"""Host restatement of the aligned crop (include/sdm.h, sdm_align_*; csrc/sdm_align.hip): the integer bilinear warp from a given
float32 crop -> source matrix in the device's float32 arithmetic (every operation rounded, nothing contracted), and a plain float64
similarity fit to check the device's matrices against.

  fit64(rows, landmark_index, template)    crop -> source matrices (N x 2 x 3, float64) and the degenerate mask
  warp(image, M, width, height)            one crop (height x width [x C] uint8) of ``image`` through the float32 matrix M
  partial(M, width, height, W, H)          the PARTIAL rule: a crop corner samples outside [0, W - 1] x [0, H - 1]
"""
import numpy as np

DEGENERATE, PARTIAL = 1, 2
f32 = np.float32
MAX_POS = f32(2.0 ** 20)


def fit64(rows, landmark_index, template):
    """The least-squares similarity (no reflection) that maps each row's selected landmarks onto the template, written plainly in
    float64, and its inverse: the crop -> source matrix.  Returns (M N x 2 x 3 float64, NaN for a degenerate row; degenerate N)."""
    rows = np.atleast_2d(np.asarray(rows, np.float32)).astype(np.float64)
    L = rows.shape[1] // 2
    idx = np.asarray(landmark_index, np.int64)
    q = np.asarray(template, np.float32).astype(np.float64).reshape(-1, 2)
    p = np.stack([rows[:, idx], rows[:, L + idx]], -1)                   # N x K x 2
    pb, qb = p.mean(1), q.mean(0)
    u, v = p - pb[:, None, :], q - qb
    spp = (u ** 2).sum((1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (u * v).sum((1, 2)) / spp
        b = (u[..., 0] * v[:, 1] - u[..., 1] * v[:, 0]).sum(1) / spp
        d = a * a + b * b
        A = np.stack([np.stack([a / d, b / d], -1), np.stack([-b / d, a / d], -1)], 1)      # N x 2 x 2
        t = pb - np.einsum("nij,j->ni", A, qb)
    M = np.concatenate([A, t[:, :, None]], 2)
    degenerate = ~np.isfinite(p).all((1, 2)) | (spp == 0)
    M[degenerate] = np.nan
    return M, degenerate


def positions(M, width, height):
    """float32 source positions of every crop pixel: sx = (M00 j + M01 i) + M02, sy likewise (height x width each)."""
    m = np.asarray(M, np.float32).reshape(2, 3)
    j = np.arange(width, dtype=f32)[None, :]
    i = np.arange(height, dtype=f32)[:, None]
    sx = (m[0, 0] * j + m[0, 1] * i) + m[0, 2]
    sy = (m[1, 0] * j + m[1, 1] * i) + m[1, 2]
    return sx.astype(f32), sy.astype(f32)


def warp(image, M, width, height):
    """One crop as the device computes it: positions quantised to 1/32 pixel, integer bilinear weights, taps outside the image 0,
    a non-finite position or one beyond 2^20 gives 0.  image: H x W or H x W x C uint8; returns height x width [x C] uint8."""
    img = np.asarray(image, np.uint8)
    gray = img.ndim == 2
    if gray:
        img = img[:, :, None]
    H, W, C = img.shape
    sx, sy = positions(M, width, height)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(sx) <= MAX_POS) & (np.abs(sy) <= MAX_POS)
    sxs, sys_ = np.where(ok, sx, f32(0)), np.where(ok, sy, f32(0))
    X = np.floor(sxs * f32(32) + f32(0.5)).astype(np.int64)
    Y = np.floor(sys_ * f32(32) + f32(0.5)).astype(np.int64)
    x0, fx, y0, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        return np.where(inside[..., None], v, 0)

    w00, w10 = ((32 - fx) * (32 - fy))[..., None], (fx * (32 - fy))[..., None]
    w01, w11 = ((32 - fx) * fy)[..., None], (fx * fy)[..., None]
    acc = w00 * tap(x0, y0) + w10 * tap(x0 + 1, y0) + w01 * tap(x0, y0 + 1) + w11 * tap(x0 + 1, y0 + 1)
    out = np.where(ok[..., None], (acc + 512) >> 10, 0).astype(np.uint8)
    return out[..., 0] if gray else out


def partial(M, width, height, W, H):
    """SDM_ALIGN_PARTIAL of one non-degenerate row: a crop corner's float32 position outside [0, W - 1] x [0, H - 1]."""
    sx, sy = positions(M, width, height)
    cx = sx[[0, 0, -1, -1], [0, -1, 0, -1]]
    cy = sy[[0, 0, -1, -1], [0, -1, 0, -1]]
    with np.errstate(invalid="ignore"):
        inside = (cx >= 0) & (cx <= f32(W - 1)) & (cy >= 0) & (cy <= f32(H - 1))
    return not inside.all()


def similarity(scale, angle_deg, tx, ty):
    """A crop -> source similarity [[s cos, -s sin, tx], [s sin, s cos, ty]] (float64)."""
    r = np.deg2rad(angle_deg)
    c, s = scale * np.cos(r), scale * np.sin(r)
    return np.array([[c, -s, tx], [s, c, ty]], np.float64)


def apply(M, pts):
    """Points (K x 2) through a 2 x 3 map, float64."""
    pts = np.asarray(pts, np.float64)
    return pts @ np.asarray(M, np.float64)[:, :2].T + np.asarray(M, np.float64)[:, 2]
