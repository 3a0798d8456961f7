"""The cases of the tracker's motion-compensated initialisation at the edges of its contract (include/sdm.h, "Tracking,
motion-compensated"): every search reach, every cell size, ties and extremes of the key, every row length, slots and rows in any order.

A controllable tracker: a one-level cascade whose regressor is all zero returns every row as its initialisation, bit for bit, so with
init "previous", min_size 0 and max_scale_change 0 a started row is align_mean(mean, box) and a tracked row its last row plus the
search's shift.  ``Tracker`` restates exactly that on tests/track_motion_ref.py (``R.Motion``, ``R.shifted``) and tests/track_ref.py; with
a device adapter (``dev``) it drives the library through the same calls and asserts, after every step, the premise -- the device's rows
are the stated rows -- the lost masks and the motion state of EVERY slot.  Each ``case_*`` function builds its frames, runs its steps and
asserts its conditions on the reference alone; tests/test_track_motion_cases_host.py runs them without a device,
tests/test_gpu_track_motion_edges.py with one.  A plain module, host only."""
import numpy as np

import landmark_count_cases as K
import track_motion_ref as R
import track_ref as T
from superviseddescent_amd import synth

f32 = np.float32
FREE, STARTED, TRACKED, LOST = 0, 1, 2, 3
SAD_MAX = 32 * 32 * 255


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid_mean(L, last=(0.0, 0.0)):
    """tests/test_gpu_track_landmark_counts.py's mean on a dyadic grid inside [-0.375, 0.375]^2: landmarks 0 and 1 hold the corners, the
    eyes sit at L - 5 ... L - 2, 0.5 apart on one line.  In a box of b pixels align_mean is exact for every b below 2^10: the body
    spans 0.75 b on both axes around the box's centre."""
    mx, my = np.empty(L, f32), np.empty(L, f32)
    k = np.arange(L)
    mx[:] = ((k * 5) % 23 - 11) / 32.0
    my[:] = ((k * 7) % 19 - 9) / 32.0
    mx[0], my[0], mx[1], my[1] = -0.375, -0.375, 0.375, 0.375
    mx[L - 5:L - 1] = [-0.25 - 1 / 64, -0.25 + 1 / 64, 0.25 - 1 / 64, 0.25 + 1 / 64]
    my[L - 5:L - 1] = -0.125
    mx[L - 1], my[L - 1] = last
    return np.concatenate([mx, my]).astype(f32)


def eyes(L):
    return [L - 5, L - 4], [L - 3, L - 2]


def cell_of(box, scale):
    """the cell size of a grid_mean face in a box of ``box`` pixels, and the quotient it is the ceiling of"""
    q = 0.75 * box * scale / 32.0
    return min(int(np.ceil(q)), R.MAX_K), q


class Scene:
    """a frame cut out of a larger buffer: frame(dx, dy) shows the content moved by exactly (dx, dy) pixels.  Smooth structure plus
    noise (tests/test_gpu_track_motion.py's Placed), or with ``block`` random levels on squares of that side plus noise, so that block
    means of that size differ from cell to cell."""

    def __init__(self, w, h, pad, seed, block=0):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.pad = w, h, pad
        H, W = h + 2 * pad, w + 2 * pad
        if block:
            levels = rng.integers(30, 226, (H // block + 2, W // block + 2))
            base = np.kron(levels, np.ones((block, block), np.int64))[block // 3:block // 3 + H, block // 2:block // 2 + W]
        else:
            yy, xx = np.mgrid[0:H, 0:W]
            base = 128 + 60 * np.sin(xx / 9.0 + rng.uniform(0, 6)) * np.cos(yy / 7.0 + rng.uniform(0, 6))
        self.buf = np.clip(base + rng.normal(0, 12, (H, W)), 0, 255).astype(np.uint8)

    def frame(self, dx=0, dy=0):
        y0, x0 = self.pad - dy, self.pad - dx
        assert 0 <= y0 and y0 + self.h <= self.buf.shape[0] and 0 <= x0 and x0 + self.w <= self.buf.shape[1]
        return np.ascontiguousarray(self.buf[y0:y0 + self.h, x0:x0 + self.w])


class Tracker:
    """the controllable tracker restated; ``dev``: None or the device adapter (configure, start, step, motion)"""

    def __init__(self, L, mean, slots, motion, mode="previous", eye_idx=None, dev=None):
        self.L, self.mean, self.mode, self.dev = L, np.asarray(mean, f32), mode, dev
        self.ref = R.Motion(slots, *motion)
        self.rows = np.zeros((slots, 2 * L), f32)
        self.status = np.zeros(slots, np.int32)
        self.boxes = np.zeros((slots, 4), np.int32)
        self.all = np.arange(slots)
        if dev is not None:
            dev.configure(L, self.mean, slots, mode, motion, eye_idx or eyes(L))
            self.check()

    def start(self, ids, boxes):
        ids = np.asarray(ids)
        self.boxes[ids] = np.asarray(boxes, np.int32).reshape(-1, 4)
        self.status[ids] = STARTED
        self.ref.invalidate(ids)
        if self.dev is not None:
            self.dev.start(ids, self.boxes[ids])

    def search(self, i, image):
        """the reference's search of slot i in ``image``, the state untouched"""
        return R.search(self.ref.chips[i], tuple(int(v) for v in self.ref.grid[i]), image, self.ref.S, self.ref.min_gain)

    def step(self, ids, images, idx=None):
        """one step of the rows ``ids``: (rows, lost masks, shifts), the state committed"""
        ids = np.asarray(ids)
        n = ids.size
        im = np.arange(n) if idx is None else np.asarray(idx)
        assert np.isin(self.status[ids], (STARTED, TRACKED)).all()
        tracked = self.status[ids] == TRACKED
        shifts = self.ref.search_step(ids, tracked, images, idx)
        moved = R.shifted(self.rows[ids], shifts)
        init = moved if self.mode == "previous" else T.realign(moved, self.mean)
        for i in np.flatnonzero(~tracked):
            init[i] = synth.align_mean(self.mean, tuple(int(v) for v in self.boxes[ids[i]]))
        res = init
        W, H = np.array([images[j].shape[1] for j in im]), np.array([images[j].shape[0] for j in im])
        lost = T.lost_mask(init, res, W, H, 0.0)
        if self.dev is not None:
            got, got_lost = self.dev.step(ids, images, idx)
            assert np.array_equal(bits(got), bits(res)), np.argwhere(bits(got) != bits(res))[:4]      # the premise
            assert np.array_equal(got_lost, lost), (got_lost, lost)
        self.rows[ids] = res
        self.status[ids] = np.where(lost != 0, LOST, TRACKED)
        self.ref.store_step(ids, res, lost, images, idx)
        self.check()
        return res, lost, shifts

    def check(self, ids=None):
        """the device's motion state of the slots ``ids`` (every slot) against the restatement's"""
        if self.dev is None:
            return
        ids = self.all if ids is None else np.asarray(ids)
        m, g, ch = self.dev.motion(ids)
        rm, rg, rch = self.ref.get(ids)
        assert np.array_equal(m, rm), (m, rm)
        assert np.array_equal(g, rg), (g, rg)
        assert np.array_equal(ch, rch), np.argwhere(ch != rch)[:4]


# ---- a. every offset's SAD ----------------------------------------------------------------------------------------------------------------

# S -> (box, scale): cell sizes 2, 3, 4, 2
REACH = {1: (64, 1.0), 5: (96, 1.25), 8: (128, 1.25), 16: (64, 1.25)}


def translations(S):
    """the chain's moves in cells: the four corners, the four edge centres, then moves of every residue of (S + dx) & 3 and, from S = 8
    on, offsets held by every one of the four waves; the running sum stays within [-S, S]"""
    t = [(S, S), (-S, -S), (S, -S), (-S, S), (0, S), (0, -S), (S, 0), (-S, 0)]
    return t + [m for m in ((3, -2), (-1, 2), (-2, 4), (1, -1), (2, 1), (-3, -4)) if max(abs(m[0]), abs(m[1])) <= S]


def case_reach(S, min_gain, dev=None):
    box, scale = REACH[S]
    k = cell_of(box, scale)[0]
    assert 2 <= k <= 4
    side = (32 + 4 * S) * k + 32
    sc = Scene(side, side, 2 * S * k + 8, 100 + S)
    L = 8
    tr = Tracker(L, grid_mean(L), 1, (S, scale, min_gain), dev=dev)
    b = (side - box) // 2
    tr.start([0], [[b, b, box, box]])
    x0 = synth.align_mean(tr.mean, (b, b, box, box))
    res, lost, _ = tr.step([0], [sc.frame()])
    assert np.array_equal(bits(res[0]), bits(x0)) and lost[0] == 0 and tr.ref.grid[0, 0] == k
    moves = translations(S)
    assert len(moves) >= 6
    at, waves, residues = np.zeros(2, np.int64), set(), set()
    for dx, dy in moves:
        at += (dx * k, dy * k)
        assert np.abs(at).max() <= S * k
        frame = sc.frame(int(at[0]), int(at[1]))
        kk, ox, oy = (int(v) for v in tr.ref.grid[0])
        # the chip and its translated copy lie wholly inside the frame
        for X, Y in ((ox, oy), (ox + dx * k, oy + dy * k)):
            assert 0 <= X and X + 32 * k <= side and 0 <= Y and Y + 32 * k <= side
        table = tr.search(0, frame)["table"]
        assert int((table == 0).sum()) == 1 and table[dy + S, dx + S] == 0            # the only zero is the translation's
        prev = tr.rows[0].copy()
        res, lost, shifts = tr.step([0], [frame])
        last = tr.ref.last[0]
        assert tuple(last) == (dx * k, dy * k, 0, last[3], k, 1) and last[3] > 0
        assert lost[0] == 0 and np.array_equal(bits(res), bits(R.shifted(prev[None], [[dx * k, dy * k]])))
        assert tuple(tr.ref.grid[0]) == (kk, ox + dx * k, oy + dy * k)
        waves.add((((dy + S) * (2 * S + 1) + dx + S) % 256) // 64)
        residues.add((S + dx) & 3)
    assert residues == {(S + d) & 3 for d in range(-S, S + 1)} and (len(residues) == 4 or S == 1)
    assert waves == {0, 1, 2, 3} or S < 8
    # the chain ends where the sum of the shifts says, bit for bit
    end = x0.copy()
    end[:L] += f32(at[0])
    end[L:] += f32(at[1])
    assert np.array_equal(bits(tr.rows[0]), bits(end))
    return dict(S=S, k=k, steps=len(moves), pitch=((32 + 2 * S + 3) & ~3) + 4)


# ---- b. cell sizes ------------------------------------------------------------------------------------------------------------------------

# scale -> boxes; the cell sizes 1, 3, 5 | 2, 8 | 63, 64 (q = 63.75), 64 (capped, q = 96)
CELLS = {1.0: (40, 128, 200), 1.25: (64, 256), 4.0: (672, 680, 1024)}
CELL_SET = [1, 2, 3, 5, 8, 63, 64, 64]
CELL_GAIN = 64
CELL_MOVE, CELL_MOVE_BIG = (3, -2), (1, 0)


def cell_move(k):
    """cells the content moves by: at k >= 63 a frame of 960 x 720 covers fifteen by eleven cells, and the border that does not move
    with the content outweighs a longer move"""
    return CELL_MOVE if k < 63 else CELL_MOVE_BIG


def case_cells(S, scale, dev=None):
    """rows of one scale on frames of 640 x 480 (960 x 720 at k >= 63: most of every chip and window still lies outside), each on its own image: the store, a step whose content moved by cell_move(k) cells of
    the row's own grid, a step whose content stays and only its noise changes.  Returns per row (k, q, shifted, refused, chip)."""
    w, h = (640, 480) if scale < 4 else (960, 720)
    boxes = CELLS[scale]
    n = len(boxes)
    ks = [cell_of(b, scale)[0] for b in boxes]
    scenes = [Scene(w, h, 3 * k + 8, 1000 * S + 7 * b, block=max(k, 4)) for b, k in zip(boxes, ks)]
    L = 8
    tr = Tracker(L, grid_mean(L), n, (S, scale, CELL_GAIN), dev=dev)
    ids = np.arange(n)
    tr.start(ids, [[(w - b) // 2, (h - b) // 2, b, b] for b in boxes])
    res, lost, _ = tr.step(ids, [s.frame() for s in scenes])
    assert not lost.any() and tr.ref.grid[:, 0].tolist() == ks
    chips = tr.ref.chips.copy()
    moved = [s.frame(cell_move(k)[0] * k, cell_move(k)[1] * k) for s, k in zip(scenes, ks)]
    res, lost, shifts = tr.step(ids, moved)
    assert not lost.any()
    shifted = (shifts != 0).any(1)
    rng = np.random.default_rng(5 + S)
    noisy = [np.clip(f.astype(int) + rng.integers(-9, 10, f.shape), 0, 255).astype(np.uint8) for f in moved]
    res, lost, shifts3 = tr.step(ids, noisy)
    last = tr.ref.last
    refused = np.array([last[i, 5] == 1 and not R.accept(last[i, 2], last[i, 3], CELL_GAIN) for i in ids])
    assert not shifts3[refused].any()
    return [(ks[i], cell_of(boxes[i], scale)[1], bool(shifted[i]), bool(refused[i]), chips[i]) for i in ids]


def cells_conditions(rows):
    """``rows``: case_cells' rows of every scale at one S"""
    assert sorted(r[0] for r in rows) == CELL_SET
    big = [r for r in rows if r[0] >= 63]
    assert len(big) <= 3
    assert sorted(r[1] for r in big)[0] == 63.0 and 63 < sorted(r[1] for r in big)[1] <= 64 and sorted(r[1] for r in big)[2] > 64
    for k in set(CELL_SET):
        assert any(r[2] for r in rows if r[0] == k), k                    # a searched row of this cell size takes a non-zero shift
        assert any(r[3] for r in rows if r[0] == k), k                    # and one is refused by min_gain
    for r in big:
        assert (r[4] == 0).any() and (r[4] != 0).any()


# ---- c. ties and extremes -----------------------------------------------------------------------------------------------------------------

def one_row(frames, box, motion, dev=None, at=None, L=8):
    """a face of ``box`` pixels in the middle of the first frame (or at ``at``), one step per frame; the tracker"""
    h, w = frames[0].shape
    tr = Tracker(L, grid_mean(L), 1, motion, dev=dev)
    x, y = at if at is not None else ((w - box) // 2, (h - box) // 2)
    tr.start([0], [[x, y, box, box]])
    for f in frames:
        res, lost, _ = tr.step([0], [f])
        assert lost[0] == 0
    return tr


def case_flat(dev=None):
    """a constant frame: every offset ties at SAD 0, the key picks (0, 0)"""
    flat = np.full((160, 160), 93, np.uint8)
    for S in (16, 5):
        tr = Tracker(8, grid_mean(8), 1, (S, 1.0, 0), dev=dev)
        tr.start([0], [[60, 60, 40, 40]])
        tr.step([0], [flat])
        table = tr.search(0, flat)["table"]
        assert table.shape == (2 * S + 1, 2 * S + 1) and not table.any()
        tr.step([0], [flat])
        assert tuple(tr.ref.last[0]) == (0, 0, 0, 0, 1, 1)


def case_ties(dev=None):
    """windows that tie at two offsets or more; k = 2, S = 5, the window of 84 pixels inside frames of 200 x 200.
    0: columns -- f(x), moved by two cells: SAD 0 at (2, dy) for every dy, the squared distances differ, (2, 0) wins;
    1: columns of period three cells, moved by one: SAD 0 at dx = 1, -2, 4, -5, the distances differ, (1, 0) wins;
    2: anti-diagonals -- f(x + y), moved by one cell: SAD 0 wherever dx + dy = 1; (1, 0) and (0, 1) lie equally far, the smaller dy wins"""
    S, k, n = 5, 2, 200
    rng = np.random.default_rng(31)
    g = rng.integers(0, 256, 3 * n).astype(np.uint8)
    yy, xx = np.mgrid[0:n, 0:n]
    per = np.tile(rng.integers(0, 256, 3 * k).astype(np.uint8), n)
    pairs = [(g[xx + 50], g[xx + 50 - 2 * k]), (per[xx + 60], per[xx + 60 - k]), (g[xx + yy + 50], g[xx + yy + 50 - k])]
    want = [(2, 0), (1, 0), (1, 0)]
    tr = Tracker(8, grid_mean(8), 3, (S, 1.25, 0), dev=dev)
    ids = np.arange(3)
    tr.start(ids, [[68, 68, 64, 64]] * 3)
    tr.step(ids, [np.ascontiguousarray(a) for a, _ in pairs])
    assert tr.ref.grid[:, 0].tolist() == [k] * 3
    second = [np.ascontiguousarray(b) for _, b in pairs]
    t = [tr.search(i, second[i])["table"] for i in ids]
    assert (t[0][:, S + 2] == 0).all() and int((t[0] == 0).sum()) == 2 * S + 1
    assert (t[1][:, [S - 5, S - 2, S + 1, S + 4]] == 0).all() and int((t[1] == 0).sum()) == 4 * (2 * S + 1)
    assert t[2][S, S + 1] == 0 and t[2][S + 1, S] == 0 and int((t[2] == 0).sum()) == 2 * S
    res, lost, shifts = tr.step(ids, second)
    assert shifts.tolist() == [[dx * k, dy * k] for dx, dy in want] and not tr.ref.last[:, 2].any() and (tr.ref.last[:, 3] > 0).all()


def case_extremes(dev=None):
    """all 255 stored, all 0 searched: every offset's SAD is 32 * 32 * 255, against the key's bit 40; (0, 0) whatever min_gain"""
    white, black = np.full((160, 160), 255, np.uint8), np.zeros((160, 160), np.uint8)
    for gain in (0, 1):
        tr = one_row([white], 40, (16, 1.0, gain), dev=dev)
        table = tr.search(0, black)["table"]
        assert (table == SAD_MAX).all() and SAD_MAX << 22 >= 1 << 39
        tr.step([0], [black])
        assert tuple(tr.ref.last[0]) == (0, 0, SAD_MAX, SAD_MAX, 1, 1)


# min_gain -> (best, zero, accepted): best * 256 exactly at, one below and one above zero * (256 - min_gain).  At min_gain 0 nothing
# lies above (best <= zero always); its first row ties everywhere, so (0, 0) is the best offset
BOUNDARIES = {0: [(300, 300, True), (299, 300, True)],
              1: [(255, 256, True), (254, 255, True), (256, 257, False)],
              255: [(2, 512, True), (1, 257, True), (1, 255, False)]}


def boundary_frames(best, zero, ox, oy, n=120):
    """k = 1, the chip's origin (ox, oy).  Stored: 100 everywhere but a few pixels of the chip that add up to ``best`` above it.  Searched:
    100 everywhere but pixels in the chip's first column that add up to ``zero - best``: an offset with dx >= 1 does not see that
    column and has the SAD ``best``, (1, 0) the nearest of them; every other offset has ``zero``."""
    a, b = np.full((n, n), 100, np.uint8), np.full((n, n), 100, np.uint8)
    left, i = best, 0
    while left > 0:
        a[oy + 7 + 2 * i, ox + 5 + 3 * i] = 100 + min(left, 100)
        left, i = left - min(left, 100), i + 1
    left, j = zero - best, 0
    while left > 0:
        b[oy + j, ox] = 100 + min(left, 100)
        left, j = left - min(left, 100), j + 1
    assert i <= 8 and j <= 32
    return a, b


def case_boundaries(gain, dev=None):
    rows = BOUNDARIES[gain]
    n, S = len(rows), 4
    tr = Tracker(8, grid_mean(8), n, (S, 1.0, gain), dev=dev)
    ids = np.arange(n)
    tr.start(ids, [[40, 40, 40, 40]] * n)
    pairs = [boundary_frames(b, z, 44, 44) for b, z, _ in rows]
    tr.step(ids, [a for a, _ in pairs])
    assert (tr.ref.grid == (1, 44, 44)).all()
    res, lost, shifts = tr.step(ids, [b for _, b in pairs])
    for i, (best, zero, taken) in enumerate(rows):
        assert tuple(tr.ref.last[i, 2:]) == (best, zero, 1, 1)
        assert (best * 256 <= zero * (256 - gain)) == taken
        assert abs(best * 256 - zero * (256 - gain)) <= (1 if gain else 256)      # (at min_gain 0 both sides are multiples of 256)
        assert shifts[i].tolist() == ([1, 0] if taken and best < zero else [0, 0])
    return shifts


# ---- d. row lengths -----------------------------------------------------------------------------------------------------------------------

LENGTHS = [2, 5, 32, 33, 64, 65, 68, 72]
LENGTH_MOVES = ((3, -2), (-2, 1))


def length_mean(L):
    """landmark_count_cases' mean with the last landmark its sole x-minimum and y-maximum"""
    mean = K.mean(L)
    mean[L - 1] = mean[:L].min() - f32(0.125)
    mean[2 * L - 1] = mean[L:].max() + f32(0.125)
    return mean


def case_length(L, mode, dev=None):
    """two rows of 2L coordinates on two frames; the content moves by LENGTH_MOVES cells of each row's own grid"""
    _, re, le = K.landmark_set(L)
    S, scale, size = 8, 1.25, 420
    scenes = [Scene(size, size, 40, 900 + L), Scene(size - 37, size - 11, 40, 901 + L)]
    tr = Tracker(L, length_mean(L), 2, (S, scale, 0), mode=mode, eye_idx=(re, le), dev=dev)
    ids = np.arange(2)
    tr.start(ids, [[120, 130, 160, 160], [100, 110, 150, 150]])
    tr.step(ids, [s.frame() for s in scenes])
    at = np.zeros((2, 2), np.int64)
    for dx, dy in LENGTH_MOVES:
        ks = tr.ref.grid[:, 0].astype(np.int64)
        assert (ks <= 10).all()
        # wherever L > 64 the store's second turn decides the grid: without the last landmark it is another
        for i in ids:
            row = tr.rows[i]
            cut = np.delete(row, [L - 1, 2 * L - 1])
            assert (row[L - 1] < row[:L - 1]).all() and (row[2 * L - 1] > row[L:2 * L - 1]).all()
            assert R.grid(cut, scale) != R.grid(row, scale)
        at += np.stack([dx * ks, dy * ks], 1)
        prev = tr.rows.copy()
        res, lost, shifts = tr.step(ids, [s.frame(int(a[0]), int(a[1])) for s, a in zip(scenes, at)])
        assert not lost.any()
        assert np.array_equal(shifts, np.stack([dx * ks, dy * ks], 1))         # sx != sy, both non-zero
        assert (shifts[:, 0] != shifts[:, 1]).all() and (shifts != 0).all() and not tr.ref.last[:, 2].any()
        if mode == "previous":
            assert np.array_equal(bits(res), bits(R.shifted(prev, shifts)))
    return tr


# ---- e. slots and rows --------------------------------------------------------------------------------------------------------------------

def case_slots(dev=None):
    """seven slots, one never stepped; ids shuffled, descending, subsets; a slot's image another one of another size from step to step;
    at last an image so small that the whole window lies outside it"""
    S, scale, k, box = 5, 1.25, 2, 64
    sizes = [(260, 240), (300, 220), (240, 280), (256, 256), (231, 247), (290, 301)]
    scenes = [Scene(w, h, 24, 60 + i) for i, (w, h) in enumerate(sizes)]
    tr = Tracker(8, grid_mean(8), 7, (S, scale, 0), dev=dev)
    order = np.array([5, 3, 4, 1, 0, 2])
    tr.start(order, [[90 + 2 * i, 80 + 3 * i, box, box] for i in order])
    frames = [s.frame() for s in scenes]
    tr.step(order, frames, idx=order)                                     # row i of the step is slot order[i] on image order[i]
    assert tr.ref.valid.tolist() == [True] * 6 + [False]
    for ids in ([6], [2], [6, 0], [3, 6, 1], [4, 6, 0, 5, 2]):            # n = 1, 2, 3, 5, permuted, with the never-stepped slot
        tr.check(ids)
    # descending, a subset: every content moved by (2, -1) cells
    moved = [s.frame(2 * k, -k) for s in scenes]
    down = np.array([5, 3, 1])
    res, lost, shifts = tr.step(down, moved, idx=down)
    assert shifts.tolist() == [[2 * k, -k]] * 3 and not lost.any()
    # shuffled, another subset; slot 4 looks at image 0 and slot 0 at image 4 (other sizes, other content)
    mixed, images = np.array([1, 4, 0, 5]), np.array([1, 0, 4, 5])
    res, lost, shifts = tr.step(mixed, [s.frame(4 * k, -2 * k) for s in scenes], idx=images)
    assert shifts[0].tolist() == [2 * k, -k] and shifts[3].tolist() == [2 * k, -k] and not lost.any()
    assert tr.ref.last[4, 2] > 0 and tr.ref.last[0, 2] > 0
    for ids in ([6], [5, 4], [0, 6, 3], [2, 0, 6, 1, 4]):
        tr.check(ids)
    # slot 3 on an image of 8 x 8: its window lies wholly outside, its chip holds the face; the row is lost there (its centre is outside)
    tiny = np.full((8, 8), 200, np.uint8)
    kk, ox, oy = (int(v) for v in tr.ref.grid[3])
    assert ox - S * kk >= 8 and oy - S * kk >= 8 and tr.ref.chips[3].any()
    window = R.block_means(tiny, ox - S * kk, oy - S * kk, kk, 32 + 2 * S)
    assert not window.any()
    res, lost, shifts = tr.step([3, 2], [tiny, frames[2]], idx=[0, 1])
    assert lost.tolist() == [T.OUTSIDE, 0] and not shifts.any()
    assert tr.ref.last[3, 2] == tr.ref.last[3, 3] > 0 and tr.ref.last[3, 5] == 1 and not tr.ref.valid[3] and tr.ref.valid[2]
    return tr


def case_many(dev=None):
    """257 slots on four shared images: all started in one step, 65 of them in the next, all 257 shuffled in the third"""
    S, scale, k, n = 5, 1.25, 2, 257
    sizes = [(320, 300), (301, 333), (280, 290), (350, 270)]
    scenes = [Scene(w, h, 16, 70 + i) for i, (w, h) in enumerate(sizes)]
    rng = np.random.default_rng(257)
    image = (np.arange(n) % 4).astype(np.int32)
    boxes = np.array([[rng.integers(40, sizes[j][0] - 104), rng.integers(40, sizes[j][1] - 104), 64, 64] for j in image], np.int32)
    tr = Tracker(8, grid_mean(8), n, (S, scale, 0), dev=dev)
    ids = np.arange(n)
    tr.start(ids, boxes)
    res, lost, _ = tr.step(ids, [s.frame() for s in scenes], idx=image)
    assert not lost.any() and (tr.ref.grid[:, 0] == k).all()
    some = ids[::-1][:65]
    res, lost, shifts = tr.step(some, [s.frame(-3 * k, 2 * k) for s in scenes], idx=image[some])
    assert not lost.any() and (shifts != 0).any(1).sum() >= 60
    every = rng.permutation(n)
    res, lost, shifts = tr.step(every, [s.frame(-2 * k, 4 * k) for s in scenes], idx=image[every])
    assert not lost.any() and (shifts != 0).any(1).sum() >= 240
    return tr
