"""The tracker's motion-compensated initialisation restated in numpy (include/sdm.h, "Tracking, motion-compensated"): the grid of a
landmark row, block means on it, the SAD table of a reference chip against a search window, the arg-min on (SAD, dx^2 + dy^2, dy, dx),
the acceptance rule, and the per-slot state a tracker keeps.  Integer throughout except the grid, which is float32 with every
operation rounded.  A plain module, imported by the tests."""
import numpy as np

f32 = np.float32
C = 32
MAX_K = 64
MAX_POS = f32(1048576.0)


def grid(row, scale):
    """(k, ox, oy) of a landmark row (2L floats)"""
    row = np.asarray(row, f32)
    L = row.size // 2
    return grid_of_bounds(row[:L].min(), row[:L].max(), row[L:].min(), row[L:].max(), scale)


def grid_of_bounds(x0, x1, y0, y1, scale):
    x0, x1, y0, y1, scale = (f32(v) for v in (x0, x1, y0, y1, scale))
    with np.errstate(all="ignore"):
        side = f32(np.fmax(f32(x1 - x0), f32(y1 - y0)) * scale)
        q = np.ceil(f32(side / f32(32.0)))
        k = MAX_K if q >= MAX_K else (int(q) if q >= 1 else 1)
        cx = np.fmin(np.fmax(f32(f32(x0 + x1) * f32(0.5)), -MAX_POS), MAX_POS)
        cy = np.fmin(np.fmax(f32(f32(y0 + y1) * f32(0.5)), -MAX_POS), MAX_POS)
    return k, int(np.floor(cx)) - 16 * k, int(np.floor(cy)) - 16 * k


def block_means(img, X0, Y0, k, n):
    """n x n uint8: (sum of the k x k taps from (X0 + i k, Y0 + j k) + k^2 / 2) / k^2, a tap outside the image 0"""
    img = np.asarray(img)
    h, w = img.shape
    sums = np.zeros((n, n), np.int64)
    xa, xb = max(X0, 0), min(X0 + n * k, w)
    ya, yb = max(Y0, 0), min(Y0 + n * k, h)
    if xa < xb and ya < yb:
        # only the cells the image overlaps are laid out (a window of 64 x 64 cells of 64 x 64 taps mostly lies outside a frame)
        ca, cb, ra, rb = (xa - X0) // k, (xb - X0 + k - 1) // k, (ya - Y0) // k, (yb - Y0 + k - 1) // k
        region = np.zeros(((rb - ra) * k, (cb - ca) * k), np.int64)
        region[ya - Y0 - ra * k:yb - Y0 - ra * k, xa - X0 - ca * k:xb - X0 - ca * k] = img[ya:yb, xa:xb]
        sums[ra:rb, ca:cb] = region.reshape(rb - ra, k, cb - ca, k).sum(axis=(1, 3))
    return ((sums + (k * k) // 2) // (k * k)).astype(np.uint8)


def store(row, img, scale):
    """the grid and the reference chip of a committed row"""
    g = grid(row, scale)
    return g, block_means(img, g[1], g[2], g[0], C)


def sad_table(chip, cur, S):
    """(2S + 1) x (2S + 1) int64, [dy + S][dx + S]"""
    win = np.lib.stride_tricks.sliding_window_view(cur.astype(np.int32), (C, C))          # [2S + 1][2S + 1][32][32]
    return np.abs(win - chip.astype(np.int32)[None, None]).sum(axis=(2, 3)).astype(np.int64)


def accept(best, zero, min_gain):
    return int(best) * 256 <= int(zero) * (256 - int(min_gain))


def search(chip, g, img, S, min_gain):
    """the search of one row in the new image: dict(table, dx, dy: the best offset in cells, best, zero, shift: pixels)"""
    k, ox, oy = g
    cur = block_means(img, ox - S * k, oy - S * k, k, C + 2 * S)
    table = sad_table(chip, cur, S)
    d = np.arange(-S, S + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    key = (table << 22) | ((dx * dx + dy * dy) << 12) | ((dy + 16) << 6) | (dx + 16)
    at = np.unravel_index(np.argmin(key), key.shape)
    bdx, bdy, best, zero = int(dx[at]), int(dy[at]), int(table[at]), int(table[S, S])
    take = accept(best, zero, min_gain)
    return dict(table=table, dx=bdx, dy=bdy, best=best, zero=zero, shift=(bdx * k, bdy * k) if take else (0, 0))


def shifted(rows, shifts):
    """rows n x 2L with the shifts n x 2 (pixels) added in float32: the landmarks as the gather reads them; a shift of (0, 0) keeps the
    row's bits"""
    rows = np.array(rows, f32, copy=True)
    L = rows.shape[1] // 2
    for i, (sx, sy) in enumerate(np.asarray(shifts).reshape(-1, 2)):
        if sx != 0 or sy != 0:
            rows[i, :L] = rows[i, :L] + f32(sx)
            rows[i, L:] = rows[i, L:] + f32(sy)
    return rows


class Motion:
    """the state of sdm_track_configure_motion over `slots` slots"""

    def __init__(self, slots, search=8, scale=1.25, min_gain=32):
        self.S, self.scale, self.min_gain = int(search), float(scale), int(min_gain)
        self.valid = np.zeros(slots, bool)
        self.grid = np.zeros((slots, 3), np.int32)
        self.chips = np.zeros((slots, C, C), np.uint8)
        self.last = np.zeros((slots, 6), np.int32)

    def invalidate(self, ids):
        self.valid[np.asarray(ids)] = False

    def search_step(self, ids, tracked, images, idx=None):
        """ahead of the gather: the rows' shifts n x 2 (pixels); tracked: per row, whether the slot's status is TRACKED"""
        shifts = np.zeros((len(ids), 2), np.int32)
        for i, id_ in enumerate(ids):
            if not (tracked[i] and self.valid[id_]):
                self.last[id_] = 0
                continue
            r = search(self.chips[id_], tuple(int(v) for v in self.grid[id_]), images[i if idx is None else idx[i]], self.S, self.min_gain)
            shifts[i] = r["shift"]
            self.last[id_] = (r["shift"][0], r["shift"][1], r["best"], r["zero"], self.grid[id_, 0], 1)
        return shifts

    def store_step(self, ids, rows, masks, images, idx=None):
        """behind the commit: rows n x 2L the committed raw rows, masks the lost masks"""
        for i, id_ in enumerate(ids):
            if masks[i] != 0:
                self.valid[id_] = False
                continue
            g, chip = store(rows[i], images[i if idx is None else idx[i]], self.scale)
            self.valid[id_], self.grid[id_], self.chips[id_] = True, g, chip

    def get(self, ids):
        ids = np.asarray(ids)
        v = self.valid[ids]
        return self.last[ids].copy(), np.where(v[:, None], self.grid[ids], 0), np.where(v[:, None, None], self.chips[ids], 0)
