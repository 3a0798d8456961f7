"""Aligned face crops on the device (csrc/sdm_align.hip, include/sdm.h sdm_align_*, detection_model.aligned_crops): every crop against
the host restatement (tests/align_ref.py) applied to the device's own matrix, the matrices against a float64 fit, identity and known
similarities, borders, degenerate rows, row independence, the tracker hand-off, the device output path, argument limits, the C++
layer, and the agreement of crops of rotated faces."""
import os

import numpy as np
import pytest

import align_ref as A
import cpp_build as B
from superviseddescent_amd import (Context, HoGParam, HogTransform, LinearRegressor, Regulariser, SdmError, SupervisedDescentOptimiser,
                                   alignment_template, detection_model, ibug, synth)

pytestmark = pytest.mark.gpu
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
SEL = np.array([ibug.IBUG68_IDS.index(i) for i in IDS] + [68 + ibug.IBUG68_IDS.index(i) for i in IDS])
PARAMS = [HoGParam(*p) for p in ibug.SHIPPED_HOG_PARAMS]
LM = np.array([3, 6, 9, 12, 15, 18, 21]) % L               # a few landmarks (eyes, nose, mouth of RCR-22)
# crops of one face rotated by up to 30 degrees, aligned on its rotated ground truth, differ from the unrotated face's crop by at most
# this mean absolute difference in the crop's central quarter: measured 6.85 (mean 4.15) over 8 faces x 4 angles
ROTATED_MAD = 8.0


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def faces():
    images, boxes, gt = synth.make_faces(16, seed=5150)
    return images, boxes, gt[:, SEL].astype(np.float32)


@pytest.fixture(scope="module")
def model(built):
    images, boxes, gt = synth.make_faces(600, seed=9200, chunk=32)
    x_star, x0, idx = synth.make_samples(boxes, gt, IDS, n_perturb=4, seed=9201)
    sdo = SupervisedDescentOptimiser([LinearRegressor(Regulariser(Regulariser.RegularisationType.MatrixNorm, 1.5, False)) for _ in PARAMS])
    sdo.train(x_star, x0, None, HogTransform(images, PARAMS, IDS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS, idx))
    return detection_model(sdo, MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def check_crops(crops, mats, flags, rows, images, idx, lm, tmpl, w, h):
    """every row: its crop is the restatement's warp through the device's M, M is the float64 fit to 1 ULP, the flags are right"""
    M64, deg = A.fit64(rows, lm, tmpl)
    for r in range(rows.shape[0]):
        img = images[idx[r]]
        if deg[r]:
            assert flags[r] == A.DEGENERATE and np.isnan(mats[r]).all() and not crops[r].any()
            continue
        ref32 = M64[r].astype(np.float32)
        tol = np.maximum(np.spacing(np.abs(ref32)), np.float32(1e-12 * np.abs(M64[r]).max()))
        assert (np.abs(mats[r].astype(np.float64) - ref32) <= tol).all(), (r, mats[r], M64[r])
        want = A.warp(img, mats[r], w, h)
        assert np.array_equal(crops[r].reshape(want.shape), want), r
        assert flags[r] == (A.PARTIAL if A.partial(mats[r], w, h, img.shape[1], img.shape[0]) else 0), r


def test_gray_context_images_of_mixed_sizes(ctx, faces):
    images, _, rows = faces
    rng = np.random.default_rng(1)
    # mixed sizes: crop / pad the 256 x 256 faces differently; rows keep their coordinates relative to the face
    imgs = [np.ascontiguousarray(images[0][:200, :230]), np.ascontiguousarray(images[1]),
            np.pad(images[2], ((10, 30), (40, 0))), np.ascontiguousarray(images[3][16:, 8:])]
    shift = np.array([[0, 0], [0, 0], [40, 10], [-8, -16]], np.float32)
    idx = np.array([0, 1, 2, 3, 1, 2])
    x = rows[[0, 1, 2, 3, 1, 2]].copy()
    for r in range(6):
        x[r, :L] += shift[idx[r], 0]
        x[r, L:] += shift[idx[r], 1]
    x[4] += rng.normal(0, 2, 2 * L).astype(np.float32)
    ctx.upload_images(imgs)
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    for (w, h) in ((112, 112), (97, 61), (1, 1), (3, 5)):
        tmpl = alignment_template(MEAN, LM, w, h, 0.2)
        ctx.align_set_source(None)
        crops, mats, flags = ctx.align_crops(LM, tmpl, w, h)
        assert crops.shape == (6, h, w, 1)
        check_crops(crops[..., 0], mats, flags, x, imgs, idx, LM, tmpl, w, h)
    ctx.set_sample_image_index(None)


def test_external_host_colour_and_device_rgba_stacks(ctx, faces):
    import torch
    images, _, rows = faces
    rng = np.random.default_rng(2)
    n = 8
    colour = rng.integers(0, 256, (n, 256, 256, 3), dtype=np.uint8)
    colour[..., 1] = images[:n]                                          # (a face in one channel)
    rgba = rng.integers(0, 256, (n, 256, 256, 4), dtype=np.uint8)
    ctx.upload_images(list(images[:n]))
    ctx.set_sample_image_index(None)
    x = rows[:n].copy()
    ctx.set_x(x)
    w, h = 112, 96
    tmpl = alignment_template(MEAN, np.arange(L), w, h, 0.15)
    assert ctx.align_set_source(colour) == 3
    crops, mats, flags = ctx.align_crops(np.arange(L), tmpl, w, h, 3)
    check_crops(crops, mats, flags, x, colour, np.arange(n), np.arange(L), tmpl, w, h)
    dev = torch.from_numpy(rgba).cuda()
    assert ctx.align_set_source(dev) == 4
    crops4, mats4, flags4 = ctx.align_crops(np.arange(L), tmpl, w, h, 4)
    check_crops(crops4, mats4, flags4, x, rgba, np.arange(n), np.arange(L), tmpl, w, h)
    assert np.array_equal(mats4.view(np.uint32), mats.view(np.uint32))
    # gray crops of the context's images are the colour crops' face channel
    ctx.align_set_source(None)
    gray, _, _ = ctx.align_crops(np.arange(L), tmpl, w, h)
    assert np.array_equal(gray[..., 0], crops[..., 1])


def test_identity_and_known_similarities(ctx, faces):
    images, _, rows = faces
    ctx.upload_images(list(images[:4]))
    ctx.set_sample_image_index(None)
    x = rows[:4].copy()
    ctx.set_x(x)
    for r in range(4):                                                   # template = the row's own landmarks, crop = the image
        t = np.stack([x[r, :L], x[r, L:]], 1)
        crops, mats, flags = ctx.align_crops(np.arange(L), t, 256, 256)
        assert np.array_equal(mats[r], np.array([[1, 0, 0], [0, 1, 0]], np.float32)) and flags[r] == 0
        assert np.array_equal(crops[r, ..., 0], images[r])
    # landmarks made from a known crop -> source similarity
    rng = np.random.default_rng(3)
    tmpl = alignment_template(MEAN, np.arange(L), 112, 112, 0.2).astype(np.float64)
    S_all, xs = [], []
    for k in range(64):
        s, a = rng.uniform(0.3, 3.0), rng.uniform(-45, 45)
        S = A.similarity(s, a, *rng.uniform(0, 256, 2))
        p = A.apply(S, tmpl)
        S_all.append(S)
        xs.append(np.concatenate([p[:, 0], p[:, 1]]))
    ctx.upload_images([images[0]] * 64)
    ctx.set_x(np.array(xs, np.float32))
    crops, mats, flags = ctx.align_crops(np.arange(L), tmpl.astype(np.float32), 112, 112)
    for k in range(64):
        assert np.abs(mats[k] - S_all[k]).max() / np.abs(S_all[k]).max() < 1e-5, k
    check_crops(crops[..., 0], mats, flags, np.array(xs, np.float32), [images[0]] * 64, np.arange(64), np.arange(L),
                tmpl.astype(np.float32), 112, 112)


def test_borders_and_degenerate_rows(ctx, faces):
    images, _, rows = faces
    ctx.upload_images(list(images[:6]))
    ctx.set_sample_image_index(None)
    x = rows[:6].copy()
    x[1, :L] += 150.0                                                    # half the face beyond the right edge
    x[2, :] = 17.0                                                       # coincident landmarks
    x[3, LM[2]] = np.nan                                                 # a selected landmark is NaN
    x[4, L:] -= 120.0                                                    # beyond the top
    tmpl = alignment_template(MEAN, LM, 112, 112, 0.2)
    ctx.set_x(rows[:6])
    clean, _, _ = ctx.align_crops(LM, tmpl, 112, 112)
    ctx.set_x(x)
    crops, mats, flags = ctx.align_crops(LM, tmpl, 112, 112)
    assert list(flags[[0, 5]]) == [0, 0] and flags[1] == A.PARTIAL and flags[4] == A.PARTIAL
    assert flags[2] == A.DEGENERATE and flags[3] == A.DEGENERATE and not crops[2].any() and not crops[3].any()
    assert np.array_equal(crops[[0, 5]], clean[[0, 5]])                  # neighbours unchanged
    for r in (1, 4):                                                     # outside pixels are 0
        sx, sy = A.positions(mats[r], 112, 112)
        out = (sx < -1) | (sx > 256) | (sy < -1) | (sy > 256)
        assert out.any() and not crops[r, ..., 0][out].any()
    check_crops(crops[..., 0], mats, flags, x, images, np.arange(6), LM, tmpl, 112, 112)


def test_rows_are_independent(ctx, faces):
    images, _, rows = faces
    n = 4096
    rng = np.random.default_rng(4)
    idx = np.arange(n) % 16
    x = rows[idx] + rng.normal(0, 3, (n, 2 * L)).astype(np.float32)
    ctx.upload_images(list(images))
    ctx.set_sample_image_index(idx)
    ctx.set_x(x)
    tmpl = alignment_template(MEAN, LM, 112, 112, 0.2)
    crops, mats, flags = ctx.align_crops(LM, tmpl, 112, 112)
    pick = [0, 1, 777, 2048, 4095]
    check_crops(crops[pick, ..., 0], mats[pick], flags[pick], x[pick], images, idx[pick], LM, tmpl, 112, 112)
    for r in pick:
        ctx.set_sample_image_index(idx[r:r + 1])
        ctx.set_x(x[r:r + 1])
        one, m1, f1 = ctx.align_crops(LM, tmpl, 112, 112)
        assert np.array_equal(one[0], crops[r]) and np.array_equal(m1[0].view(np.uint32), mats[r].view(np.uint32)) and f1[0] == flags[r]
    ctx.set_sample_image_index(None)


def test_after_tracker_step_and_out_tensor(model):
    import torch
    frames, _, boxes = synth.make_tracks(6, 3, seed=82)
    S = frames.shape[1]
    ids = np.arange(S)
    tmpl = alignment_template(MEAN, LM, 112, 112, 0.2)

    def run(with_crops):
        tr = model.tracker(S, init="realign")
        tr.start(ids, boxes[0])
        out = []
        for t in range(3):
            res, _ = tr.step(ids, list(frames[t]))
            if with_crops and t < 2:
                crops, mats, flags = model.aligned_crops(112, [IDS[i] for i in LM], tmpl)
                lm, _ = tr.get(ids)
                check_crops(crops[..., 0], mats, flags, lm, frames[t], ids, LM, tmpl, 112, 112)
                dev = torch.zeros((S, 112, 112, 1), dtype=torch.uint8, device="cuda")
                got, mats2, _ = model.aligned_crops(112, [IDS[i] for i in LM], tmpl, out=dev)
                assert got is dev and np.array_equal(dev.cpu().numpy(), crops) and np.array_equal(mats2, mats)
            out.append(res)
        return np.stack(out)

    assert np.array_equal(run(True).view(np.uint32), run(False).view(np.uint32))     # crops do not disturb the tracker


def test_argument_limits(ctx, faces):
    import torch
    images, _, rows = faces
    ctx.upload_images(list(images[:4]))
    ctx.set_sample_image_index(None)
    ctx.set_x(rows[:4])
    tmpl = alignment_template(MEAN, LM, 32, 32, 0.2)
    good = ctx.align_crops(LM, tmpl, 32, 32)
    INVALID = -1
    lib, h = ctx._lib, ctx._h
    cases = [
        lambda: ctx.align_crops(LM[:1], tmpl[:1], 32, 32),                               # K < 2
        lambda: ctx.align_crops(np.arange(L + 1) % L, np.zeros((L + 1, 2)), 32, 32),     # K > L (and repeated)
        lambda: ctx.align_crops([0, 0], tmpl[:2], 32, 32),                               # repeated
        lambda: ctx.align_crops([0, L], tmpl[:2], 32, 32),                               # out of range
        lambda: ctx.align_crops([0, -1], tmpl[:2], 32, 32),
        lambda: ctx.align_crops(LM, np.full_like(tmpl, 3.0), 32, 32),                    # coincident template
        lambda: ctx.align_crops(LM, np.where(np.arange(LM.size)[:, None] == 1, np.nan, tmpl), 32, 32),
        lambda: ctx.align_crops(LM, tmpl, 0, 32),
        lambda: ctx.align_crops(LM, tmpl, 32, 1025),
        lambda: ctx.align_set_source(np.zeros((4, 256, 256, 2), np.uint8)),              # channels
        lambda: ctx.align_crops(LM, tmpl, 32, 32, out=torch.zeros(4 * 32 * 32 + 1, dtype=torch.uint8, device="cuda")[1:].view(4, 32, 32, 1)),   # misaligned
        lambda: lib.sdm_align_set_source(h, images.ctypes.data, 4, 256, 256, 255, 1, 0) and _raise(lib),   # stride < width
        lambda: lib.sdm_align_set_source(h, images.ctypes.data, 0, 256, 256, 256, 1, 0) and _raise(lib),
    ]
    for f in cases:
        assert code(f) == INVALID
        assert all(np.array_equal(a, b) for a, b in zip(ctx.align_crops(LM, tmpl, 32, 32), good))
    # sources that do not cover the rows: too few images, the wrong size, an index beyond
    ctx.align_set_source(np.zeros((3, 256, 256, 3), np.uint8))
    assert code(ctx.align_crops, LM, tmpl, 32, 32, 3) == INVALID
    ctx.align_set_source(np.zeros((4, 255, 256, 3), np.uint8))
    assert code(ctx.align_crops, LM, tmpl, 32, 32, 3) == INVALID
    ctx.align_set_source(None)
    ctx.set_sample_image_index([0, 1, 2, 3, 3])
    ctx.upload_images(list(images[:3]))
    assert code(ctx.align_crops, LM, tmpl, 32, 32) == INVALID
    ctx.upload_images(list(images[:4]))
    ctx.set_sample_image_index(None)
    fresh = Context(0)
    try:
        assert code(fresh.align_crops, LM, tmpl, 32, 32) == INVALID                     # no geometry, no rows
    finally:
        fresh.close()
    assert all(np.array_equal(a, b) for a, b in zip(ctx.align_crops(LM, tmpl, 32, 32), good))


def test_output_must_match_the_source_channels(ctx, faces):
    """the library writes N x H x W x C bytes of the installed source: a buffer sized for another C is refused before any launch"""
    import torch
    images, _, rows = faces
    ctx.upload_images(list(images[:4]))
    ctx.set_sample_image_index(None)
    ctx.set_x(rows[:4])
    tmpl = alignment_template(MEAN, LM, 32, 32, 0.2)
    colour = np.repeat(images[:4, :, :, None], 3, axis=3)
    assert ctx.align_set_source(colour) == 3 and ctx.align_channels == 3
    crops, _, _ = ctx.align_crops(LM, tmpl, 32, 32)                                     # C taken from the source
    assert crops.shape == (4, 32, 32, 3)
    with pytest.raises(ValueError):
        ctx.align_crops(LM, tmpl, 32, 32, 1)
    for bad in (torch.zeros((4, 32, 32, 1), dtype=torch.uint8, device="cuda"),           # C of a gray source
                torch.zeros((4, 32, 32 * 3), dtype=torch.uint8, device="cuda"),           # right size, wrong shape
                torch.zeros((4, 32, 32, 3), dtype=torch.int8, device="cuda")):            # not uint8
        with pytest.raises(ValueError):
            ctx.align_crops(LM, tmpl, 32, 32, out=bad)
    with pytest.raises(ValueError):
        ctx.align_set_source(torch.zeros((4, 256, 256, 3), dtype=torch.int8, device="cuda"))
    assert ctx.align_channels == 3
    dev = torch.zeros((4, 32, 32, 3), dtype=torch.uint8, device="cuda")
    ctx.align_crops(LM, tmpl, 32, 32, out=dev)
    assert np.array_equal(dev.cpu().numpy(), crops)
    assert ctx.align_set_source(None) == 1 and ctx.align_crops(LM, tmpl, 32, 32)[0].shape == (4, 32, 32, 1)


def _raise(lib):
    raise SdmError(-1, lib.sdm_last_error().decode())


def test_rotated_faces_agree(ctx):
    images, _, gt = synth.make_faces(8, seed=4242)
    angles = [-30, -15, 0, 15, 30]
    tmpl = alignment_template(MEAN, np.arange(L), 112, 112, 0.2)
    rot_imgs, rows = [], []
    for f in range(8):
        r0 = gt[f][SEL].astype(np.float64)
        c = np.array([r0[:L].mean(), r0[L:].mean()])
        for a in angles:
            fwd = A.similarity(1.0, a, 0, 0)
            fwd[:, 2] = c - fwd[:, :2] @ c
            inv = A.similarity(1.0, -a, 0, 0)
            inv[:, 2] = c - inv[:, :2] @ c
            rot_imgs.append(A.warp(images[f], inv.astype(np.float32), 256, 256))
            p = A.apply(fwd, np.stack([r0[:L], r0[L:]], 1))
            rows.append(np.concatenate([p[:, 0], p[:, 1]]))
    ctx.upload_images(rot_imgs)
    ctx.set_sample_image_index(None)
    ctx.set_x(np.array(rows, np.float32))
    crops, _, flags = ctx.align_crops(np.arange(L), tmpl, 112, 112)
    crops = crops[..., 0].reshape(8, len(angles), 112, 112).astype(np.float64)
    ref = crops[:, angles.index(0)]
    mad = [np.abs(crops[f, k, 28:84, 28:84] - ref[f, 28:84, 28:84]).mean() for f in range(8) for k in range(len(angles)) if angles[k]]
    print("rotated faces: central MAD max %.3f mean %.3f" % (max(mad), np.mean(mad)))
    assert max(mad) <= ROTATED_MAD


def test_cpp_alignment_matches_python(model, tmp_path):
    frames, _, boxes = synth.make_tracks(4, 2, seed=83)
    n_frames, S, H, W = frames.shape
    colour = np.random.default_rng(5).integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    colour[..., 0] = frames[1]
    d = str(tmp_path)
    B.write_model(d, L, model.hog_params, MEAN, IDS, regressors=[r.x for r in model.optimised_model.regressors])
    frames.tofile(os.path.join(d, "frames.u8"))
    colour.tofile(os.path.join(d, "colour.u8"))
    boxes.astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    LMl = [int(v) for v in LM]
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{S} {n_frames} {H} {W} {len(LMl)} " + " ".join(map(str, LMl)) + "\n")
    B.run(B.gpu_driver("align_gpu", tmp_path), [d], 300)
    # the same through Python: the tracker after two frames (gray and colour), and detect_batch's rows on frame 0
    tmpl = alignment_template(MEAN, LM, 112, 112, 0.2)
    names = [IDS[i] for i in LM]
    tr = model.tracker(S)
    ids = np.arange(S)
    tr.start(ids, boxes[0])
    tr.step(ids, list(frames[0]))
    tr.step(ids, list(frames[1]))
    g, gm, gf = model.aligned_crops(112, names, tmpl)
    c3, _, _ = model.aligned_crops(112, names, tmpl, source=colour)
    rows = model.detect_batch(list(frames[0]), boxes[0])
    dcrops, dm, _ = model.aligned_crops(112, names, tmpl)
    cpp = lambda name, dt, shape: np.fromfile(os.path.join(d, name), dt).reshape(shape)
    assert np.array_equal(cpp("track_gray.u8", np.uint8, g.shape), g)
    assert np.array_equal(cpp("track_mats.f32", np.float32, (S, 2, 3)).view(np.uint32), gm.view(np.uint32))
    assert np.array_equal(cpp("track_flags.i32", np.int32, (S,)), gf)
    assert np.array_equal(cpp("track_colour.u8", np.uint8, c3.shape), c3)
    assert np.array_equal(cpp("detect_rows.f32", np.float32, rows.shape).view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(cpp("detect_gray.u8", np.uint8, dcrops.shape), dcrops)
    assert np.array_equal(cpp("detect_mats.f32", np.float32, (S, 2, 3)).view(np.uint32), dm.view(np.uint32))
