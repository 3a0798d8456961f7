"""Piecewise-affine warped faces on the device (csrc/sdm_warp.hip, csrc/sdm_capi_warp.hip; include/sdm.h "Warped faces";
detection_model.warped_crops_tensor).  State comes from set_model_geometry and set_x.  The label map and the matrices are compared bit for
bit with the float64 restatement (tests/warp_ref.py), the elements bit for bit with the restatement applied to the device's own matrices."""
import ctypes
import itertools

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import warp_cases as W
import warp_ref as R
from superviseddescent_amd import Context, HoGParam, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, ibug, synth

pytestmark = pytest.mark.gpu
IDS, L, MEAN = W.IDS, W.L, W.MEAN
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
MESHES = {"rcr22": W.mesh_rcr22, "single": W.mesh_single, "254": W.mesh_254}


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = W.place()
    return buf, frames, [K.host_frame(buf, f) for f in frames]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def device_frames(buf, frames, names=K.NAMES):
    import torch
    dev = torch.from_numpy(buf).cuda()
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], names[f["fmt"]]) for f in frames]
    chroma = [base + f["uv_off"] if f["fmt"] == T.NV12 else None for f in frames]
    return dev, lst, chroma


def install(ctx, buf, frames, rows, x, names=K.NAMES):
    """frames as the context's images and as the crop source, the rows; returns what must stay alive"""
    dev, lst, chroma = device_frames(buf, frames, names)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(rows)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, chroma=chroma)
    return dev, lst, chroma


def restore(ctx):
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def sizes(frames, rows):
    return [(frames[i]["w"], frames[i]["h"]) for i in rows]


def check_call(ctx, host, rows, lab, cache, **spec):
    """one call against the restatement on the device's own matrices; cache: the warped pixels per row (independent of the spec)"""
    out, mats, flags = ctx.warp_crops_tensor(**spec)
    got = out.cpu().numpy()
    for r, im in enumerate(rows):
        m = mats[r].reshape(-1, 6)
        if r not in cache:
            cache[r] = (m.copy(),) + R.warped(host[im], m, lab)
        m0, kind, bgr, y = cache[r]
        assert np.array_equal(bits(m0), bits(m)), r
        want = T.finish(kind, bgr, y, **spec)
        assert got[r].dtype == want.dtype and got[r].shape == want.shape
        assert np.array_equal(bits(got[r]), bits(want)), (r, host[im].fmt, spec)
    return out, mats, flags


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_labels_and_matrices(ctx, placed, mesh):
    buf, frames, host = placed
    for (w, h) in W.CROPS:
        idx, t, tri = MESHES[mesh](w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        assert lab.shape == (h, w) and np.array_equal(lab, R.labels(t, tri, w, h))
        assert (lab == R.NONE).any() and (lab != R.NONE).any()
        x = W.rows_for(frames, W.ROWS, idx, t, w, h, 3)
        keep = install(ctx, buf, frames, W.ROWS, x)
        out, mats, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=1)
        assert mats.shape == (len(W.ROWS), len(tri), 2, 3)
        # fixed-order IEEE double on both sides, nothing contracted: equality is the expectation
        assert np.array_equal(bits(mats.reshape(len(W.ROWS), -1, 6)), bits(R.matrices(x, idx, t, tri)))
        assert np.array_equal(flags, R.flags(x, idx, t, tri, sizes(frames, W.ROWS)))
        assert np.array_equal(keep[0].cpu().numpy(), buf)                 # the in-place source is only read
    restore(ctx)


@pytest.mark.parametrize("mesh", ["rcr22", "254"])
def test_elements_odd_crop_every_combination(ctx, placed, mesh):
    buf, frames, host = placed
    w, h = W.CROPS[1]
    idx, t, tri = MESHES[mesh](w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = W.rows_for(frames, W.ROWS, idx, t, w, h, 40)
    keep = install(ctx, buf, frames, W.ROWS, x)
    cache = {}
    for dtype, layout, channels, order in COMBOS if mesh == "rcr22" else COMBOS[::5]:
        check_call(ctx, host, W.ROWS, lab, cache, dtype=dtype, layout=layout, channels=channels, order=order, scale=SCALES, bias=BIASES,
                   gray_shift=14 if order == "bgr" else 15)
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_elements_every_source_format(ctx, placed):
    buf, frames, host = placed
    w, h = W.CROPS[0]
    # the same bytes read as (gray, bgr, rgba, nv12) and as (gray, rgb, bgra, nv12): all six formats
    swapped = {**K.NAMES, T.BGR: "rgb", T.RGBA: "bgra"}
    host2 = [T.Frame({T.BGR: T.RGB, T.RGBA: T.BGRA}.get(f.fmt, f.fmt), f.pix, f.uv) for f in host]
    specs = [dict(dtype="float16", layout="nchw", channels=3, order="rgb", scale=SCALES, bias=BIASES),
             dict(dtype="uint8", layout="nhwc", channels=1, gray_shift=15)]
    for name, fn in sorted(MESHES.items()):
        idx, t, tri = fn(w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        x = W.rows_for(frames, W.ROWS, idx, t, w, h, 41)
        for names, hosts in ((K.NAMES, host), (swapped, host2)):
            keep = install(ctx, buf, frames, W.ROWS, x, names)
            cache = {}
            for spec in specs:
                check_call(ctx, hosts, W.ROWS, lab, cache, **spec)
    restore(ctx)


def identity_mesh(w, h):
    """8 template points on a quarter-pixel grid and their Delaunay triangles, every |D| >= 1"""
    rng = np.random.default_rng(4)
    t = (rng.integers(4, 4 * np.array([w, h]) - 4, (8, 2)) / 4.0).astype(np.float32)
    tri = _lib.delaunay(t)
    assert (np.abs(R.constants(t, tri)[2]) >= 1).all()
    return np.arange(8) * 2 + 1, t, tri


def test_identity(ctx, placed):
    """landmarks = template + an integer translation: every labelled pixel IS the source pixel, without any restatement"""
    buf, frames, host = placed
    w, h = W.CROPS[0]
    idx, t, tri = identity_mesh(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    on = lab != R.NONE
    assert on.sum() > 60 and (~on).any()
    shifts = [(5, 7), (11, 3), (0, 0), (13, 12)]                           # (24 + 13 <= 37, 20 + 12 <= 33: inside every frame)
    rows = [0, 1, 2, 1]
    x = np.zeros((4, 2 * L), np.float32)
    for r, (tx, ty) in enumerate(shifts):
        x[r, idx], x[r, L + idx] = t[:, 0] + tx, t[:, 1] + ty
    keep = install(ctx, buf, frames, rows, x)
    out, mats, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=3, order="bgr")
    got = out.cpu().numpy()
    assert not flags.any()
    for r, (tx, ty) in enumerate(shifts):
        pix = host[rows[r]].pix
        src = pix[ty:ty + h, tx:tx + w]
        src = np.repeat(src[..., None], 3, -1) if src.ndim == 2 else src[..., :3][..., ::-1] if host[rows[r]].fmt == T.RGBA else src
        assert np.array_equal(got[r][on], src[on]) and not got[r][~on].any(), r
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_agrees_with_the_similarity_crop(ctx):
    """K = 3, T = 1, landmarks an exact similarity image of the template: inside the triangle the warp and sdm_align_crops_tensor on the
    same three points differ by at most 1 level.  Both sample the same map up to float32 rounding of two differently computed matrices, so
    a position may fall on neighbouring 1/32 steps of either axis; on a source whose neighbouring pixels differ by at most 5 levels (the
    ramp below) that moves the blend by at most 2 * 5 / 32 < 1 before rounding, hence at most 1 level after.
    Measured with the two restatements on the CPU (tests/warp_ref.py against tests/align_tensor_ref.py on align_ref.fit64's matrix,
    the 24 x 20 and 33 x 17 crops, 6 similarities each): 0 of 2 346 labelled pixels differ at all."""
    jj, ii = np.meshgrid(np.arange(48), np.arange(40))
    img = (2 * jj + 3 * ii).astype(np.uint8)
    ctx.upload_images([img])
    ctx.align_set_source(None)
    for (w, h) in W.CROPS:
        idx, t, tri = W.mesh_single(w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        on = ctx.warp_labels() != R.NONE
        sims = [A.similarity(s, a, tx, ty) for s, a, tx, ty in ((1.0, 0, 3, 4), (0.8, 20, 14, 2), (1.3, -30, 2, 18), (0.5, 45, 20, 6), (1.1, 7, 5.3, 3.7),
                                                                (0.9, -12, 8.1, 9.9))]
        x = K.landmark_rows(sims, t, idx, L)
        ctx.set_sample_image_index(np.zeros(len(sims), np.int32))
        ctx.set_x(x)
        warp, _, flags = ctx.warp_crops_tensor(dtype="uint8", layout="nhwc", channels=1)
        crop, _, _ = ctx.align_crops_tensor(idx, t, w, h, dtype="uint8", layout="nhwc", channels=1)
        a, b = warp.cpu().numpy()[..., 0].astype(int), crop.cpu().numpy()[..., 0].astype(int)
        assert not flags.any()                  # (every landmark inside the frame, so the triangle: no tap meets the 0 outside the ramp)
        diff = np.abs(a - b)[:, on]
        print("crop %d x %d: %d of %d labelled pixels differ, largest difference %d" % (w, h, (diff > 0).sum(), diff.size, diff.max()))
        assert b[:, on].any() and diff.max() <= 1
    ctx.set_sample_image_index(None)


def test_flags(ctx, placed):
    buf, frames, host = placed
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    rows = [2, 2, 2, 2, 2]                                                 # the 48 x 40 frame holds the whole template at (12, 10)
    x = np.zeros((5, 2 * L), np.float32)
    x[:, idx], x[:, L + idx] = t[:, 0] + 12, t[:, 1] + 10
    a, b, c = tri[0]
    x[0, idx[4]] = np.nan                                                   # DEGENERATE
    x[1, idx[a]] = -0.5                                                     # PARTIAL (and nothing else: see below)
    x[2, [idx[b], idx[c]]], x[2, [L + idx[b], L + idx[c]]] = x[2, [idx[c], idx[b]]], x[2, [L + idx[c], L + idx[b]]]      # FOLDED: two swapped
    x[3, idx[b]], x[3, L + idx[b]] = x[3, idx[a]], x[3, L + idx[a]]         # FOLDED: a source triangle without area
    want = R.flags(x, idx, t, tri, sizes(frames, rows))
    keep = install(ctx, buf, frames, rows, x)
    spec = dict(dtype="float32", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    out, mats, flags = ctx.warp_crops_tensor(**spec)
    got = out.cpu().numpy()
    assert np.array_equal(flags, want)
    assert flags[0] == R.DEGENERATE and flags[2] == R.FOLDED and flags[3] == R.FOLDED and flags[4] == 0
    assert flags[1] & R.PARTIAL and not flags[1] & R.DEGENERATE
    assert np.isnan(mats[0]).all() and np.isfinite(mats[1:]).all() and np.isfinite(got).all()
    for ch in range(3):
        assert np.array_equal(bits(got[0, ch]), bits(np.full((h, w), T.element(0, SCALES[ch], BIASES[ch], "float32"))))
    # PARTIAL alone: a landmark that leaves the frame without turning a triangle over -- the whole face half a pixel past the left edge
    y = x[4:5].copy()
    y[0, idx] = t[:, 0] - t[:, 0].min() - 0.5
    ctx.set_sample_image_index(rows[:1])
    ctx.set_x(y)
    assert ctx.warp_crops_tensor(**spec)[2][0] == R.PARTIAL
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def random_model():
    rng = np.random.default_rng(77)
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, p in zip(regs, PARAMS):
        reg.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)


def test_state_is_untouched_and_no_source_stays_behind(built):
    import torch
    model = random_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    rng = np.random.default_rng(5)
    colour = [np.repeat(frames[1, s][..., None], 3, -1) + rng.integers(0, 2, frames[1, s].shape + (3,), dtype=np.uint8) for s in range(2)]
    ids = np.arange(2)
    tr = model.tracker(2)
    tr.start(ids, boxes[0])
    tr.step(ids, [torch.from_numpy(f).cuda() for f in frames[0]])
    dev = [torch.from_numpy(c).cuda() for c in colour]
    tr.step(ids, dev)
    c = model.optimised_model.ctx
    lm = [IDS[i] for i in (3, 6, 9, 12, 15)]
    before = (c.get_x(), tr.get(ids), model.aligned_crops_tensor(16, lm, dtype="uint8"))
    out, mats, flags = model.warped_crops_tensor((24, 20), frames=dev, order="bgr", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    assert tuple(out.shape) == (2, 3, 20, 24) and out.dtype == torch.float16 and mats.shape[0] == 2 and mats.shape[2:] == (2, 3)
    mask = model.warp_mask()
    assert mask.shape == (20, 24) and mask.dtype == bool and mask.any() and not mask.all()
    lab = c.warp_labels()
    spec = _lib.align_tensor_spec(order="bgr", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    for s in range(2):
        want = R.tensor(T.Frame(T.BGR, colour[s]), mats[s].reshape(-1, 6), lab, order="bgr", scale=np.array(spec.scale, np.float32),
                        bias=np.array(spec.bias, np.float32))
        assert np.array_equal(bits(out[s]), bits(want))
        assert np.array_equal(dev[s].cpu().numpy(), colour[s])
    after = (c.get_x(), tr.get(ids), model.aligned_crops_tensor(16, lm, dtype="uint8"))      # the crop source is the context's images again
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(bits(before[1][0]), bits(after[1][0])) and np.array_equal(before[1][1], after[1][1])
    for p, q in zip(before[2], after[2]):
        assert np.array_equal(bits(p), bits(q))
    c.close()


def test_refusals(ctx, placed):
    import torch
    buf, frames, host = placed
    w, h = W.CROPS[0]
    idx, t, tri = W.mesh_rcr22(w, h)
    idx, tri = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(tri, np.int32)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    x = W.rows_for(frames, W.ROWS, idx, t, w, h, 9)
    dev, lst, chroma = install(ctx, buf, frames, W.ROWS, x)
    spec = dict(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    good = ctx.warp_crops_tensor(**spec) + (ctx.warp_labels(),)

    def same():
        now = ctx.warp_crops_tensor(**spec) + (ctx.warp_labels(),)
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(now, good))

    lib, hnd = ctx._lib, ctx._h

    def mesh(lm=idx, tm=t, k=None, tr=tri, nt=None, ww=w, hh=h):
        lm, tm, tr = np.ascontiguousarray(lm, np.int32), np.ascontiguousarray(tm, np.float32), np.ascontiguousarray(tr, np.int32)
        rc = lib.sdm_warp_set_mesh(hnd, lm.ctypes.data, tm.ctypes.data, len(lm) if k is None else k, tr.ctypes.data, len(tr) if nt is None else nt, ww, hh)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def tm_with(k, v):
        out = t.copy()
        out[k] = v
        return out

    cases = [
        lambda: mesh(k=2), lambda: mesh(lm=np.arange(L + 1), tm=np.zeros((L + 1, 2)), k=L + 1),                     # K outside [3, L]
        lambda: mesh(lm=np.where(np.arange(L) == 3, L, idx)), lambda: mesh(lm=np.where(np.arange(L) == 3, -1, idx)),  # an index out of range
        lambda: mesh(lm=np.where(np.arange(L) == 3, 4, idx)),                                                       # ... or repeated
        lambda: mesh(tm=tm_with(5, (np.nan, 1.0))), lambda: mesh(tm=tm_with(0, (1.0, np.inf))),                     # template not finite
        lambda: mesh(nt=0), lambda: mesh(tr=np.concatenate([tri] * 8)[:255]),                                       # T outside [1, 254]
        lambda: mesh(tr=np.where(np.arange(len(tri))[:, None] == 2, [0, 1, L], tri)), lambda: mesh(tr=np.where(np.arange(len(tri))[:, None] == 2, [0, -1, 2], tri)),
        lambda: mesh(tr=np.where(np.arange(len(tri))[:, None] == 2, [4, 7, 4], tri)),                               # a position twice
        lambda: mesh(tm=np.tile(np.arange(L, dtype=np.float32)[:, None], 2)),                                       # D == 0: all points on one line
        lambda: mesh(tm=np.full((L, 2), 3e38, np.float32) * np.where(np.arange(L)[:, None] % 2, 1, -1)),            # (the largest float32 differences: D stays finite in double, and is 0)
        lambda: mesh(ww=0), lambda: mesh(hh=1025), lambda: mesh(ww=1025), lambda: mesh(hh=0),
    ]
    for f in cases:
        assert code(f) == -1
        assert same()
    assert lib.sdm_warp_set_mesh(hnd, None, t.ctypes.data, L, tri.ctypes.data, len(tri), w, h) == -1 and same()
    # the warp call: what sdm_align_crops_tensor refuses of spec, out_dev and the source
    out = torch.zeros((len(W.ROWS), 3, h, w), dtype=torch.float16, device="cuda")
    mis = torch.zeros(out.numel() + 4, dtype=torch.float16, device="cuda")[4:]                                      # 8 bytes off

    def raw(spec_ptr, out_ptr):
        rc = lib.sdm_warp_crops_tensor(hnd, spec_ptr, ctypes.c_void_p(out_ptr), None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def S(**kw):
        s = _lib.align_tensor_spec(**dict(spec, **{k: v for k, v in kw.items() if k in ("scale", "bias")}))
        for k, v in kw.items():
            if k not in ("scale", "bias"):
                setattr(s, k, v)
        return ctypes.byref(s)

    calls = [lambda: raw(None, out.data_ptr()), lambda: raw(S(dtype=3), out.data_ptr()), lambda: raw(S(layout=2), out.data_ptr()),
             lambda: raw(S(order=-1), out.data_ptr()), lambda: raw(S(channels=2), out.data_ptr()), lambda: raw(S(gray_shift=13), out.data_ptr()),
             lambda: raw(S(scale=[1, np.nan, 1]), out.data_ptr()), lambda: raw(S(bias=[0, 0, np.inf]), out.data_ptr()),
             lambda: raw(S(), 0), lambda: raw(S(), mis.data_ptr())]
    for f in calls:
        assert code(f) == -1
        assert same()
    raw(S(), out.data_ptr())
    assert np.array_equal(bits(out), bits(good[0]))
    ctx.align_set_source_frames(lst[:3], chroma=chroma[:3])                 # a source that does not cover the rows
    assert code(ctx.warp_crops_tensor, **spec) == -1
    wrong = list(lst)
    wrong[1] = (lst[1][0], lst[1][1] - 1, lst[1][2], lst[1][3], lst[1][4])  # ... or differs in size from the context's image
    ctx.align_set_source_frames(wrong, chroma=chroma)
    assert code(ctx.warp_crops_tensor, **spec) == -1
    ctx.align_set_source_frames(lst, chroma=chroma)
    assert same()
    # no geometry, no mesh, no rows; another L drops the mesh
    fresh = Context(0)
    try:
        assert fresh._lib.sdm_warp_set_mesh(fresh._h, idx.ctypes.data, t.ctypes.data, L, tri.ctypes.data, len(tri), w, h) == -1      # no geometry
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        assert code(fresh.warp_crops_tensor, **spec) == -1 and code(fresh.warp_labels) == -1                                         # no mesh
        fresh.warp_set_mesh(idx, t, tri, w, h)
        assert code(fresh.warp_crops_tensor, **spec) == -1                                                                         # no rows
        fresh.set_model_geometry(L + 1, RE, LE, PARAMS)
        assert code(fresh.warp_labels) == -1
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        assert code(fresh.warp_labels) == -1
    finally:
        fresh.close()
    restore(ctx)


def test_behind_tracker_step_and_detect_batch(built):
    import torch
    model = random_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    ids = np.arange(2)
    tr = model.tracker(2)
    tr.start(ids, boxes[0])
    c = model.optimised_model.ctx
    kw = dict(dtype="float32", channels=1)
    for step in range(2):
        dev = [torch.from_numpy(f).cuda() for f in frames[step]]
        rows, lost = tr.step(ids, dev)
        a = model.warped_crops_tensor(24, **kw)
        assert np.array_equal(bits(c.get_x()), bits(rows))
        c.set_x(c.get_x())
        b = model.warped_crops_tensor(24, **kw)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
        assert np.isfinite(a[1]).all() and a[0].cpu().numpy().any()
    rows = model.detect_batch(list(frames[1]), boxes[1])
    a = model.warped_crops_tensor((33, 17), **kw)
    c = model.optimised_model.ctx
    assert np.array_equal(bits(c.get_x()), bits(rows))
    c.set_x(c.get_x())
    b = model.warped_crops_tensor((33, 17), **kw)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
    lab = c.warp_labels()
    for s in range(2):
        want = R.tensor(T.Frame(T.GRAY, frames[1][s]), a[1][s].reshape(-1, 6), lab, **kw)
        assert np.array_equal(bits(a[0][s]), bits(want))
    c.close()
