"""The tracker's motion kernels (csrc/sdm_track_motion.hip, csrc/sdm_track_motion_device.h) at the edges of their contract, on the device:
the cases of tests/track_motion_cases.py, whose conditions tests/test_track_motion_cases_host.py proves on the restatement alone, run
through Context.track_configure_motion, track_step and track_get_motion on a one-level cascade whose regressor is all zero.  After
every step the device's rows must be the stated rows (the premise), and the shifts, grids, chips and last results of EVERY slot the
restatement's (tests/track_motion_ref.py), bit for bit.

* every search reach S = 1, 5, 8, 16: chains of exact translations to all four corners and edge centres of [-S, S]^2, every residue of
  (S + dx) & 3, offsets of all four waves; the windows' pitches 40, 48, 52 and 68 bytes;
* cell sizes 1, 2, 3, 5, 8, 63, 64 and the cap, at S = 16 and S = 8;
* ties (the distance, then dy, then dx), the largest SAD, min_gain at its boundaries;
* rows of 2 ... 72 landmarks in the previous, realign and upright modes: the second turns of the gather and of the store's bounds;
* ids shuffled, descending and in subsets, a slot's image changing, a window wholly outside its image, 65 and 257 rows in one step;
* planar, P010 and described NV12 frames in one image set.

profiles/track_motion_edges.txt lists, mutation by mutation, which of these tests fail on a library whose arithmetic is changed."""
import numpy as np
import pytest

import landmark_count_cases as K
import track_motion_cases as C
import track_motion_ref as R
import track_ref as T
import upright_ref as U
from superviseddescent_amd import HoGParam

pytestmark = pytest.mark.gpu
f32 = np.float32
HP = HoGParam(1, 5, 6, 4, 0.25)
MODES = {"previous": 0, "realign": 1}


class Dev:
    """the device side of track_motion_cases.Tracker: one level, a zero regressor, no size and no scale rule"""

    def __init__(self, c):
        self.c, self.installed = c, False

    def configure(self, L, mean, slots, mode, motion, eye_idx):
        c = self.c
        c.set_detect_path(fused=True if 2 * L <= 64 else "wide")
        c.set_model_geometry(L, *eye_idx, [HP])
        c.set_regressor(0, np.zeros((c.feature_dim(0), 2 * L), f32))
        c.track_configure(slots, mean, MODES[mode], 0.0, 0.0)
        c.track_configure_motion(*motion)

    def start(self, ids, boxes):
        self.c.track_start(ids, boxes)

    def step(self, ids, images, idx):
        if not self.installed:                                         # (else the caller's frames are the image set already)
            self.c.upload_images(images)
        self.c.set_sample_image_index(idx)
        return self.c.track_step(ids)

    def motion(self, ids):
        return self.c.track_get_motion(ids)


@pytest.fixture
def dev(gpu_ctx):
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_templates(None)
    if getattr(gpu_ctx, "track_upright", False):
        gpu_ctx.track_configure_upright(False)
    yield Dev(gpu_ctx)
    if getattr(gpu_ctx, "track_upright", False):
        gpu_ctx.track_configure_upright(False)
    gpu_ctx.set_detect_path(fused=True, split_store=False)
    gpu_ctx.set_sample_image_index(None)
    gpu_ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- a. every offset's SAD ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gain", [255, 0])
@pytest.mark.parametrize("S", [1, 5, 8, 16])
def test_every_reach(dev, S, gain):
    print(C.case_reach(S, gain, dev))


# ---- b. cell sizes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", list(C.CELLS))
@pytest.mark.parametrize("S", [16, 8])
def test_every_cell_size(dev, S, scale):
    rows = C.case_cells(S, scale, dev)
    assert [r[0] for r in rows] == [C.cell_of(b, scale)[0] for b in C.CELLS[scale]]
    print([r[:4] for r in rows])


# ---- c. ties and extremes -----------------------------------------------------------------------------------------------------------------

def test_ties(dev):
    C.case_flat(dev)
    C.case_ties(dev)


def test_largest_sad(dev):
    C.case_extremes(dev)


@pytest.mark.parametrize("gain", [0, 1, 255])
def test_min_gain_boundaries(dev, gain):
    C.case_boundaries(gain, dev)


# ---- d. row lengths -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["previous", "realign"])
@pytest.mark.parametrize("L", C.LENGTHS)
def test_every_row_length(dev, L, mode):
    C.case_length(L, mode, dev)


def test_upright_row_of_65_landmarks(dev):
    """the upright set-up reads the shifted landmarks of a row of 130 coordinates: two steps restated with tests/upright_ref.py the way
    tests/test_gpu_track_motion.py does at RCR-22; the first step's rows are taken from the device"""
    L, S, scale, chip = 65, 8, 1.25, 288
    c = dev.c
    _, re, le = K.landmark_set(L)
    mean = C.length_mean(L)
    dev.configure(L, mean, 2, "realign", (S, scale, 0), (re, le))
    c.upright_configure(chip, 36)
    c.track_configure_upright(True)
    c.track_configure_motion(S, scale, 0)
    scenes = [C.Scene(420, 420, 40, 965), C.Scene(383, 409, 40, 966)]
    ref = R.Motion(2, S, scale, 0)
    ids = np.arange(2)
    c.track_start(ids, [[120, 130, 160, 160], [100, 110, 150, 150]])
    frames = [s.frame() for s in scenes]
    c.upload_images(frames)
    prev, lost = c.track_step(ids)
    assert not lost.any()
    ref.store_step(ids, prev, lost, frames)
    at = np.zeros((2, 2), np.int64)
    for dx, dy in C.LENGTH_MOVES:
        ks = ref.grid[:, 0].astype(np.int64)
        for row in prev:                                                # the store's second turn decides the grid
            assert R.grid(np.delete(row, [L - 1, 2 * L - 1]), scale) != R.grid(row, scale)
        at += np.stack([dx * ks, dy * ks], 1)
        frames = [s.frame(int(a[0]), int(a[1])) for s, a in zip(scenes, at)]
        shifts = ref.search_step(ids, np.ones(2, bool), frames)
        assert np.array_equal(shifts, np.stack([dx * ks, dy * ks], 1)) and (shifts[:, 0] != shifts[:, 1]).all() and (shifts != 0).all()
        moved = R.shifted(prev, shifts)
        Mr, Wr = U.track_setup(moved, re, le, chip)
        init = U.track_init(moved, Wr, mean)
        c.upload_images(frames)
        res, lost = c.track_step(ids)
        M, flags = c.upright_get()
        assert np.array_equal(C.bits(M), C.bits(Mr))
        assert np.array_equal(C.bits(res), C.bits(U.back(Mr, init)))    # (a zero regressor: the chip rows are their initialisation)
        W, H = np.array([f.shape[1] for f in frames]), np.array([f.shape[0] for f in frames])
        assert np.array_equal(lost, T.lost_mask(init, res, W, H, 0.0)) and not lost.any()
        ref.store_step(ids, res, lost, frames)
        m, g, ch = c.track_get_motion(ids)
        rm, rg, rch = ref.get(ids)
        assert np.array_equal(m, rm) and np.array_equal(g, rg) and np.array_equal(ch, rch)
        prev = res


# ---- e. slots and rows --------------------------------------------------------------------------------------------------------------------

def test_ids_in_any_order_and_images_that_change(dev):
    C.case_slots(dev)


def test_65_and_257_rows_in_one_step(dev):
    C.case_many(dev)


# ---- f. colour sets -----------------------------------------------------------------------------------------------------------------------

def test_planar_p010_and_described_nv12_in_one_image_set(dev):
    """three rows on a planar 3 x H x W frame, a P010 surface and an "nv12:bt709:full" frame; the gray images are the image set's own
    (download_image), the content of every frame moves by (2, -1) cells between the steps"""
    import torch
    S, scale, k, box = 5, 1.25, 2, 64
    sizes = [(240, 200), (222, 180), (200, 230)]
    scenes = [C.Scene(w, h, 16, 80 + i) for i, (w, h) in enumerate(sizes)]
    c = dev.c
    keep = []

    def install(dx, dy):
        out, fmts = [], []
        for i, (s, (w, h)) in enumerate(zip(scenes, sizes)):
            g = s.frame(dx, dy)
            if i == 0:
                t = torch.from_numpy(np.stack([g, g, g])).cuda()
                out.append(t), fmts.append("bgr_planar")
            elif i == 1:
                stride, rows = 2 * w + 6, h + (h + 1) // 2
                words = np.full((rows, stride // 2), 512 << 6, np.uint16)
                words[:h, :w] = g.astype(np.uint16) << 8                # a 10-bit sample of 4 v: its gray byte is v
                t = torch.from_numpy(words.view(np.uint8).reshape(rows, stride)).cuda()
                out.append((t.data_ptr(), w, h, stride, "p010")), fmts.append(None)
            else:
                stride, rows = w + 5, h + (h + 1) // 2
                buf = np.full((rows, stride), 128, np.uint8)
                buf[:h, :w] = g
                t = torch.from_numpy(buf).cuda()
                out.append((t.data_ptr(), w, h, stride, "nv12:bt709:full")), fmts.append(None)
            keep.append(t)
        c.set_frames_device(out, formats=fmts)
        grays = [c.download_image(i) for i in range(3)]
        assert [g.shape for g in grays] == [(h, w) for w, h in sizes]
        return grays

    tr = C.Tracker(8, C.grid_mean(8), 3, (S, scale, 0), dev=dev)
    dev.installed = True
    ids = np.arange(3)
    tr.start(ids, [[80, 60, box, box], [70, 50, box, box], [60, 80, box, box]])
    grays = install(0, 0)
    assert all(np.array_equal(g, s.frame()) for g, s in zip(grays, scenes))
    res, lost, _ = tr.step(ids, grays)
    assert not lost.any() and (tr.ref.grid[:, 0] == k).all()
    res, lost, shifts = tr.step(ids, install(2 * k, -k))
    assert shifts.tolist() == [[2 * k, -k]] * 3 and not lost.any() and not tr.ref.last[:, 2].any()
