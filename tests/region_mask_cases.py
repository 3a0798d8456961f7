"""The shared cases of the landmark region mask tests (tests/test_region_mask_host.py, tests/test_gpu_region_mask.py): crop sizes,
parameter sets, and GROUPS of rows -- a group is one region structure (sizes, holes, hull bits) with several rows of points, so that one
call draws them all.  Points are given in CROP space and carried into the frame through each row's M; rows whose vertices must land
exactly (pixel centres, pixel rows, duplicates, collinear triples) use an M of small integers, whose W and positions are exact.  The
restatement's result per (group, crop) is computed once and kept (expected)."""
import functools

import numpy as np

import align_ref as A
import region_mask_ref as R

f32 = np.float32
# 1 x 1 ... 131 x 3: the 4-byte pieces and their ends; 67 x 63 and 112 x 112: the 16-byte pieces (4221 bytes: every map begins off a piece)
CROPS = [(1, 1), (5, 7), (16, 16), (37, 29), (131, 3), (67, 63), (112, 112)]
GROWS = (0.0, 2.5, -1.5)
FEATHERS = (0.0, 0.5, 4.0, 16.0)
PARAMS = [(g, f) for g in GROWS for f in FEATHERS]
IDENTITY = np.array([1, 0, 0, 0, 1, 0], f32)
SHIFT = np.array([1, 0, 3, 0, 1, -2], f32)                               # exact: integer translation
TURN = np.array([0, -2, 5, 2, 0, 1], f32)                                # exact: a quarter turn, scale 2


def to_frame(M, crop_points):
    """the frame points (P x 2 float32) whose image under W is -- exactly, for an M of small integers and quarter-pixel points -- crop_points"""
    m = np.asarray(M, np.float64).reshape(2, 3)
    return A.apply(m, crop_points).astype(f32)


def ring(cx, cy, rx, ry, n, phase=0.0, reverse=False):
    a = phase + 2 * np.pi * np.arange(n) / n
    if reverse:
        a = a[::-1]
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1)


def sim(w, h, seed):
    """a crop -> frame similarity, scale 0.5 ... 2.5, any angle, as float32"""
    rng = np.random.default_rng(seed)
    return A.similarity(rng.uniform(0.5, 2.5), rng.uniform(-180, 180), rng.uniform(0, 300), rng.uniform(0, 300)).astype(f32).reshape(6)


def groups(w, h):
    """[(name, sizes, n_holes, hull_bits, [(M six float32, frame points P x 2 float32), ...]), ...] for a crop of w x h"""
    cx, cy, rx, ry = (w - 1) / 2, (h - 1) / 2, max(w, 3) * 0.4, max(h, 3) * 0.4
    q = lambda pts: np.round(np.asarray(pts, np.float64) * 4) / 4       # quarter pixels: exact under the integer matrices
    out = []
    # one triangle: counter-clockwise, clockwise, all vertices equal, all collinear, on pixel centres and pixel rows, far outside, +-10^6
    tri = q([[cx - rx, cy - ry], [cx + rx, cy], [cx - rx / 2, cy + ry]])
    centre = np.array([[1, 1], [w - 2, 1], [1, h - 2]], np.float64)
    on_rows = np.array([[0.5, 0], [w - 0.5, max(h - 1, 1)], [0.5, max(h - 1, 1)]], np.float64)
    rows = [(sim(w, h, 1), tri), (sim(w, h, 2), tri[::-1]), (IDENTITY, tri), (SHIFT, tri[::-1]), (TURN, tri),
            (IDENTITY, np.repeat([[cx, cy]], 3, 0)), (SHIFT, q([[cx - rx, cy - ry], [cx, cy], [cx + rx, cy + ry]])),
            (IDENTITY, centre), (TURN, centre[::-1]), (SHIFT, on_rows),
            (IDENTITY, tri + [5 * w + 300, 0]), (IDENTITY, np.array([[-1e6, -1e6], [1e6, -1e6], [0, 1e6]])),
            (IDENTITY, np.array([[-1e6, cy], [1e6, cy + 0.25], [cx, 1e6]]))]
    out.append(("triangle", [3], 0, 0, rows))
    # a 27-vertex outline with a 12-vertex hole
    outline = lambda s, rev=False: np.concatenate([ring(cx, cy, rx, ry, 27, 0.1 * s, rev), ring(cx + rx / 4, cy - ry / 5, rx / 3, ry / 3, 12, 0.2, not rev)])
    out.append(("outline_hole", [27, 12], 1, 0, [(sim(w, h, 10 + s), outline(s, s % 2 == 1)) for s in range(3)] + [(IDENTITY, q(outline(3)))]))
    # two polygons: disjoint squares; a bow-tie beside a square; overlapping squares of opposite orientation
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    two = [np.concatenate([sq(0, 0, cx - 1, cy), sq(cx + 1, cy, w, h)]),
           np.concatenate([q([[cx - rx, cy - ry], [cx + rx, cy + ry], [cx + rx, cy - ry], [cx - rx, cy + ry]]), sq(0, 0, 2, 2)]),
           np.concatenate([sq(1, 1, cx + 2, cy + 2), sq(cx - 1, cy - 1, w - 1, h - 1)[::-1]])]
    out.append(("two", [4, 4], 0, 0, [(IDENTITY, two[0]), (SHIFT, two[1]), (TURN, two[2]), (sim(w, h, 20), two[1])]))
    # a polygon and a hole: the hole inside, across the edge, outside every polygon
    holes = [np.concatenate([sq(1, 1, w - 2, h - 2), sq(cx - 1, cy - 1, cx + 2, cy + 1)]),
             np.concatenate([sq(1, 1, cx, h - 2), sq(cx - 2, cy - 2, w, cy + 2)]),
             np.concatenate([sq(0, 0, cx, cy), sq(cx + 2, cy + 2, w + 3, h + 3)])]
    out.append(("hole", [4, 4], 1, 0, [(IDENTITY, holes[0]), (SHIFT, holes[1]), (IDENTITY, holes[2]), (sim(w, h, 30), holes[0])]))
    # the hull of 22 points: random; with duplicates and collinear triples; collapsing to two points; to one
    rng = np.random.default_rng(40 + w)
    cloud = q(np.stack([rng.uniform(cx - rx, cx + rx, 22), rng.uniform(cy - ry, cy + ry, 22)], 1))
    grid = np.array([[cx - 2 + (k % 5), cy - 2 + (k // 5 % 3) * 2] for k in range(22)], np.float64)      # a 5 x 3 lattice, every point doubled
    line = np.stack([np.full(22, cx), cy + (np.arange(22) % 2) * 3.0], 1)
    out.append(("hull22", [22], 0, 1, [(sim(w, h, 41), cloud), (IDENTITY, cloud), (SHIFT, grid), (TURN, grid[::-1]), (IDENTITY, line),
                                     (SHIFT, np.repeat([[cx, cy]], 22, 0)), (IDENTITY, q(ring(cx, cy, rx, ry, 22)))]))
    # three polygons: a hull, a plain one, and a hull as the hole
    mix = np.concatenate([q(ring(cx, cy, rx, ry, 6)), sq(0, 0, 3, 2), q(ring(cx, cy, rx / 2, ry / 2, 5, 0.3, True))])
    out.append(("mixed", [6, 4, 5], 1, 0b101, [(IDENTITY, mix), (sim(w, h, 50), mix)]))
    return [(name, sizes, nh, bits, [(np.asarray(M, f32).reshape(6), to_frame(M, p)) for M, p in rows]) for name, sizes, nh, bits, rows in out]


@functools.lru_cache(maxsize=None)
def expected(w, h, name):
    """(s per row (None: flagged), flags, vertex lists) of one group at one crop size: the restatement, computed once"""
    _, sizes, nh, bits, rows = next(g for g in groups(w, h) if g[0] == name)
    return [R.row_state(M, p, sizes, nh, bits, w, h) for M, p in rows]


def expected_maps(w, h, name, grow, feather):
    """N x h x w uint8 and the flags"""
    st = expected(w, h, name)
    return (np.stack([np.zeros((h, w), np.uint8) if s is None else R.bytes_of(s, grow, feather) for s, _, _ in st]),
            np.array([f for _, f, _ in st], np.int32))


def guarded(n_bytes, seed=7):
    """(noise buffer with 64 guard bytes before and after n_bytes, the slice of the payload)"""
    buf = np.random.default_rng(seed).integers(1, 256, n_bytes + 128, dtype=np.uint8)
    return buf, slice(64, 64 + n_bytes)
