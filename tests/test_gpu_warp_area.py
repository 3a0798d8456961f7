"""Piecewise-affine warped faces with area-averaged sampling on the device (csrc/sdm_warp_area.hip, csrc/sdm_capi_warp.hip; include/sdm.h
"Warped faces, filtered"; Context.warp_crops_tensor(filter=...), detection_model.warped_crops_tensor(filter=...)).  The scaffolding is
tests/test_gpu_warp.py's: state from set_model_geometry and set_x, the samples and the elements compared bit for bit with the restatement
(tests/warp_area_ref.py) applied to the device's own matrices, the source buffer compared as a whole after the calls."""
import ctypes
import itertools

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import warp_area_cases as C
import warp_area_ref as WA
import warp_ref as R
from superviseddescent_amd import (Context, HoGParam, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, align_filter, detection_model,
                                   ibug, synth)

pytestmark = pytest.mark.gpu
IDS, L, MEAN = C.IDS, C.L, C.MEAN
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
AREA = align_filter("area")


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def placed():
    buf, frames = C.place()
    return buf, frames, [K.host_frame(buf, f) for f in frames]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def install(ctx, buf, frames, rows, x, names=K.NAMES):
    """frames as the context's images and as the crop source, the rows; returns what must stay alive"""
    import torch
    dev = torch.from_numpy(buf).cuda()
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], names[f["fmt"]]) for f in frames]
    chroma = [base + f["uv_off"] if f["fmt"] == T.NV12 else None for f in frames]
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(rows)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, chroma=chroma)
    return dev, lst, chroma


def restore(ctx):
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def want_samples(mats, flags, filt):
    """the restatement's (Sx, Sy) of the device's own matrices: N x T x 2"""
    return np.stack([WA.samples(m.reshape(-1, 6), bool(f & R.DEGENERATE), filt.mode, filt.max_samples, filt.min_scale)
                     for m, f in zip(mats, flags)])


def check_call(ctx, host, rows, lab, cache, filt=AREA, **spec):
    """one filtered call against the restatement on the device's own matrices; cache: the warped pixels per row (independent of the spec)"""
    out, mats, flags, smp = ctx.warp_crops_tensor(filter=filt, **spec)
    got = out.cpu().numpy()
    want = want_samples(mats, flags, filt)
    assert smp.dtype == np.int32 and smp.shape == want.shape and np.array_equal(smp, want)
    for r, im in enumerate(rows):
        m = mats[r].reshape(-1, 6)
        if r not in cache:
            cache[r] = (m.copy(),) + WA.warped(host[im], m, lab, want[r])
        m0, kind, bgr, y = cache[r]
        assert np.array_equal(bits(m0), bits(m)), r
        w = T.finish(kind, bgr, y, **spec)
        assert got[r].dtype == w.dtype and got[r].shape == w.shape
        assert np.array_equal(bits(got[r]), bits(w)), (r, host[im].fmt, spec)
    return out, mats, flags, smp


@pytest.mark.parametrize("mesh", ["rcr22", "254"])
def test_elements_odd_crop_every_combination(ctx, placed, mesh):
    """every dtype x layout x channels x order on the Delaunay mesh, every fifth on 254 triangles: the LDS bound with the 8-word record"""
    buf, frames, host = placed
    w, h = C.CROPS[1]
    idx, t, tri = C.MESHES[mesh](w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
    keep = install(ctx, buf, frames, C.ROWS, x)
    cache = {}
    for dtype, layout, channels, order in COMBOS if mesh == "rcr22" else COMBOS[::5]:
        out, mats, flags, smp = check_call(ctx, host, C.ROWS, lab, cache, dtype=dtype, layout=layout, channels=channels, order=order,
                                           scale=SCALES, bias=BIASES, gray_shift=14 if order == "bgr" else 15)
    assert len({tuple(p) for p in smp.reshape(-1, 2)}) >= 6 and (smp[:, :, 0] != smp[:, :, 1]).any()
    assert any(len({tuple(p) for p in row}) >= 2 for row in smp) and (smp[0] == 1).all() and flags[3] & R.PARTIAL
    assert np.array_equal(keep[0].cpu().numpy(), buf)                     # the in-place source is only read
    restore(ctx)


def test_elements_every_source_format(ctx, placed):
    buf, frames, host = placed
    w, h = C.CROPS[0]
    # the same bytes read as (gray, bgr, rgba, nv12) and as (gray, rgb, bgra, nv12): all six formats
    swapped = {**K.NAMES, T.BGR: "rgb", T.RGBA: "bgra"}
    host2 = [T.Frame({T.BGR: T.RGB, T.RGBA: T.BGRA}.get(f.fmt, f.fmt), f.pix, f.uv) for f in host]
    specs = [dict(dtype="float16", layout="nchw", channels=3, order="rgb", scale=SCALES, bias=BIASES),
             dict(dtype="uint8", layout="nhwc", channels=1, gray_shift=15)]
    for name, fn in sorted(C.MESHES.items()):
        idx, t, tri = fn(w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        lab = ctx.warp_labels()
        x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
        for names, hosts in ((K.NAMES, host), (swapped, host2)):
            keep = install(ctx, buf, frames, C.ROWS, x, names)
            cache = {}
            for spec in specs:
                check_call(ctx, hosts, C.ROWS, lab, cache, **spec)
            assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_identity_with_the_unfiltered_call(ctx, placed):
    """mode BILINEAR, max_samples = 1, and rows whose triangles are all (1, 1): the bits of sdm_warp_crops_tensor"""
    buf, frames, host = placed
    for (w, h) in C.CROPS:
        idx, t, tri = C.MESHES["rcr22"](w, h)
        ctx.warp_set_mesh(idx, t, tri, w, h)
        x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
        keep = install(ctx, buf, frames, C.ROWS, x)
        for spec in (dict(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES), dict(dtype="uint8", layout="nhwc", channels=1)):
            plain = ctx.warp_crops_tensor(**spec)
            assert len(plain) == 3
            full = ctx.warp_crops_tensor(filter="area", **spec)
            assert (full[3] > 1).any() and not np.array_equal(bits(full[0]), bits(plain[0]))      # (the rows do minify)
            for filt in ("bilinear", align_filter("bilinear", 7, 2.0), align_filter("area", 1, 1.0), align_filter("area", 16, 1e30)):
                got = ctx.warp_crops_tensor(filter=filt, **spec)
                assert len(got) == 4 and (got[3] == 1).all() and got[3].shape == (len(C.ROWS), len(tri), 2)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], plain))
            # mode AREA: the rows the restatement puts at (1, 1) throughout, in one call with rows above 1
            ones = (want_samples(full[1], full[2], AREA) == 1).all((1, 2))
            assert ones.any() and not ones.all()
            assert np.array_equal(bits(full[0])[ones], bits(plain[0])[ones])
        assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_stripes(ctx):
    """No restatement: one triangle (1, 1), (17, 1), (1, 17), landmarks 4 q + (tx, ty) on vertical 0 / 255 stripes of period 2.  G is
    diag(1 / 16) and E diag(64), so A_t = [[4, 0, tx], [0, 4, ty]] exactly (t = p_a - 4 q_a) and Sx = Sy = 4; every sub-sample sits on a half
    pixel between a 0 and a 255 column, q = 512 * 255, so every labelled pixel is (16 * 512 * 255 + 512 * 16) / (1024 * 16) = 128.  The
    unfiltered call samples integer positions: 0 or 255."""
    img = np.zeros((120, 128), np.uint8)
    img[:, 1::2] = 255
    ctx.upload_images([img])
    ctx.align_set_source(None)
    w, h = C.CROPS[0]
    idx = np.array([2, 7, 11])
    q = np.array([[1, 1], [17, 1], [1, 17]], np.float32)
    ctx.warp_set_mesh(idx, q, np.array([[0, 1, 2]], np.int32), w, h)
    on = ctx.warp_labels() != R.NONE
    assert on.sum() > 100 and (~on).any()
    shifts = [(9, 5), (30, 22), (12, 40)]
    x = np.zeros((len(shifts), 2 * L), np.float32)
    for r, (tx, ty) in enumerate(shifts):
        x[r, idx], x[r, L + idx] = 4 * q[:, 0] + tx, 4 * q[:, 1] + ty
    ctx.set_sample_image_index(np.zeros(len(shifts), np.int32))
    ctx.set_x(x)
    spec = dict(dtype="uint8", layout="nhwc", channels=1)
    out, mats, flags, smp = ctx.warp_crops_tensor(filter="area", **spec)
    plain = ctx.warp_crops_tensor(**spec)[0].cpu().numpy()[..., 0]
    got = out.cpu().numpy()[..., 0]
    assert not flags.any() and (smp == 4).all()
    for r, (tx, ty) in enumerate(shifts):
        assert np.array_equal(mats[r, 0], np.array([[4, 0, tx], [0, 4, ty]], np.float32))
        assert (got[r][on] == 128).all() and not got[r][~on].any()
        assert set(np.unique(plain[r][on])) <= {0, 255}
    ctx.set_sample_image_index(None)


def test_cap_and_min_scale(ctx, placed):
    buf, frames, host = placed
    w, h = C.CROPS[0]
    idx, t, tri = C.MESHES["rcr22"](w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
    keep = install(ctx, buf, frames, C.ROWS, x)
    spec = dict(dtype="uint8", layout="nhwc", channels=3, order="bgr")
    full = ctx.warp_crops_tensor(filter="area", **spec)[3]
    assert (full == 4).any() and (full >= 5).any()
    # the cap: rows that want 4 and 5 get 3, and the elements are the restatement's at 3
    capped = check_call(ctx, host, C.ROWS, lab, {}, align_filter("area", 3, 1.0), **spec)[3]
    assert np.array_equal(capped, np.minimum(full, 3)) and (capped[full >= 4] == 3).all()
    # the gate: a count below 2 x (value < 4) falls back to 1, next to counts in the same row that stay
    gated = check_call(ctx, host, C.ROWS, lab, {}, align_filter("area", 16, 2.0), **spec)[3]
    assert np.array_equal(gated[full >= 3], full[full >= 3]) and (gated[full == 1] == 1).all()
    assert ((gated == 1) & (full == 2)).any() and not ((gated == 2) & (full == 2)).all()
    assert any((row == 1).any() and (row > 1).any() for row in gated)
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_flags(ctx, placed):
    buf, frames, host = placed
    w, h = C.CROPS[0]
    idx, t, tri = C.MESHES["rcr22"](w, h)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    lab = ctx.warp_labels()
    rows = [2, 2, 2, 2, 2]                                                 # 128 x 120: the template at 3.5 x with room around it
    x = np.zeros((5, 2 * L), np.float32)
    x[:, idx], x[:, L + idx] = 3.5 * t[:, 0] + 20, 3.5 * t[:, 1] + 25
    a, b, c = tri[0]
    x[0, idx[4]] = np.nan                                                   # DEGENERATE
    x[1, idx] -= x[1, idx].min() + 0.5                                      # PARTIAL: the face half a pixel past the left edge
    x[2, [idx[b], idx[c]]], x[2, [L + idx[b], L + idx[c]]] = x[2, [idx[c], idx[b]]], x[2, [L + idx[c], L + idx[b]]]      # FOLDED: two swapped
    x[3, idx[b]], x[3, L + idx[b]] = x[3, idx[a]], x[3, L + idx[a]]         # FOLDED: a source triangle without area
    want = R.flags(x, idx, t, tri, [(frames[i]["w"], frames[i]["h"]) for i in rows])
    keep = install(ctx, buf, frames, rows, x)
    spec = dict(dtype="float32", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    out, mats, flags, smp = check_call(ctx, host, rows, lab, {}, **spec)    # PARTIAL and FOLDED rows follow the formula
    got = out.cpu().numpy()
    assert np.array_equal(flags, want)
    assert flags[0] == R.DEGENERATE and flags[1] == R.PARTIAL and flags[2] & R.FOLDED and flags[3] & R.FOLDED and flags[4] == 0
    assert np.isnan(mats[0]).all() and np.isfinite(mats[1:]).all() and np.isfinite(got).all()
    assert (smp[0] == 1).all() and (smp[4] == 4).all() and (smp[1:] >= 1).all() and (smp[2] != smp[4]).any()
    for ch in range(3):
        assert np.array_equal(bits(got[0, ch]), bits(np.full((h, w), T.element(0, SCALES[ch], BIASES[ch], "float32"))))
    assert np.array_equal(keep[0].cpu().numpy(), buf)
    restore(ctx)


def test_refusals(ctx, placed):
    import torch
    buf, frames, host = placed
    w, h = C.CROPS[0]
    idx, t, tri = C.MESHES["rcr22"](w, h)
    idx, tri = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(tri, np.int32)
    ctx.warp_set_mesh(idx, t, tri, w, h)
    x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
    dev, lst, chroma = install(ctx, buf, frames, C.ROWS, x)
    spec = dict(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    good = ctx.warp_crops_tensor(filter="area", **spec) + (ctx.warp_labels(),)

    def same():
        now = ctx.warp_crops_tensor(filter="area", **spec) + (ctx.warp_labels(),)
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(now, good))

    lib, hnd = ctx._lib, ctx._h
    out = torch.zeros((len(C.ROWS), 3, h, w), dtype=torch.float16, device="cuda")
    mis = torch.zeros(out.numel() + 4, dtype=torch.float16, device="cuda")[4:]                                      # 8 bytes off

    def raw(spec_ptr, filter_ptr, out_ptr):
        rc = lib.sdm_warp_crops_tensor_filtered(hnd, spec_ptr, filter_ptr, ctypes.c_void_p(out_ptr), None, None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def S(**kw):
        s = _lib.align_tensor_spec(**dict(spec, **{k: v for k, v in kw.items() if k in ("scale", "bias")}))
        for k, v in kw.items():
            if k not in ("scale", "bias"):
                setattr(s, k, v)
        return ctypes.byref(s)

    def F(mode=1, max_samples=16, min_scale=1.0):
        return ctypes.byref(_lib.SdmAlignFilter(mode, max_samples, min_scale))

    # the filter: NULL, an unknown mode, max_samples outside [1, 16], min_scale not finite or below 1
    calls = [lambda: raw(S(), None, out.data_ptr()), lambda: raw(S(), F(mode=2), out.data_ptr()), lambda: raw(S(), F(mode=-1), out.data_ptr()),
             lambda: raw(S(), F(max_samples=0), out.data_ptr()), lambda: raw(S(), F(max_samples=17), out.data_ptr()),
             lambda: raw(S(), F(min_scale=np.nan), out.data_ptr()), lambda: raw(S(), F(min_scale=np.inf), out.data_ptr()),
             lambda: raw(S(), F(min_scale=0.5), out.data_ptr())]
    # what sdm_warp_crops_tensor refuses of spec and out_dev
    calls += [lambda: raw(None, F(), out.data_ptr()), lambda: raw(S(dtype=3), F(), out.data_ptr()), lambda: raw(S(layout=2), F(), out.data_ptr()),
              lambda: raw(S(order=-1), F(), out.data_ptr()), lambda: raw(S(channels=2), F(), out.data_ptr()),
              lambda: raw(S(gray_shift=13), F(), out.data_ptr()), lambda: raw(S(scale=[1, np.nan, 1]), F(), out.data_ptr()),
              lambda: raw(S(bias=[0, 0, np.inf]), F(), out.data_ptr()), lambda: raw(S(), F(), 0), lambda: raw(S(), F(), mis.data_ptr())]
    for f in calls:
        assert code(f) == -1
        assert same()
    assert not out.cpu().numpy().any()                                      # nothing was launched
    raw(S(), F(), out.data_ptr())
    assert np.array_equal(bits(out), bits(good[0]))
    with pytest.raises(ValueError):
        ctx.warp_crops_tensor(filter="box", **spec)
    with pytest.raises(ValueError):
        ctx.warp_crops_tensor(filter=3, **spec)
    # ... and of the source
    ctx.align_set_source_frames(lst[:3], chroma=chroma[:3])                 # a source that does not cover the rows
    assert code(ctx.warp_crops_tensor, filter="area", **spec) == -1
    wrong = list(lst)
    wrong[1] = (lst[1][0], lst[1][1] - 1, lst[1][2], lst[1][3], lst[1][4])  # ... or differs in size from the context's image
    ctx.align_set_source_frames(wrong, chroma=chroma)
    assert code(ctx.warp_crops_tensor, filter="area", **spec) == -1
    ctx.align_set_source_frames(lst, chroma=chroma)
    assert same()
    # no mesh, no rows
    fresh = Context(0)
    try:
        fresh.set_model_geometry(L, RE, LE, PARAMS)
        assert code(fresh.warp_crops_tensor, filter="area", **spec) == -1                                               # no mesh
        fresh.warp_set_mesh(idx, t, tri, w, h)
        assert code(fresh.warp_crops_tensor, filter="area", **spec) == -1                                               # no rows
    finally:
        fresh.close()
    assert np.array_equal(dev.cpu().numpy(), buf)
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
    kw = dict(frames=dev, order="bgr", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    plain = model.warped_crops_tensor((24, 20), **kw)
    assert len(plain) == 3
    out, mats, flags, smp = model.warped_crops_tensor((24, 20), filter="area", **kw)
    assert tuple(out.shape) == (2, 3, 20, 24) and out.dtype == torch.float16 and smp.shape == mats.shape[:2] + (2,) and smp.dtype == np.int32
    assert np.array_equal(bits(mats), bits(plain[1])) and np.array_equal(flags, plain[2])
    lab = c.warp_labels()
    spec = _lib.align_tensor_spec(order="bgr", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
    want_s = want_samples(mats, flags, AREA)
    assert np.array_equal(smp, want_s) and (smp > 1).any()                  # (the synthetic faces are larger than 24 x 20)
    for s in range(2):
        want = WA.tensor(T.Frame(T.BGR, colour[s]), mats[s].reshape(-1, 6), lab, want_s[s], order="bgr", scale=np.array(spec.scale, np.float32),
                         bias=np.array(spec.bias, np.float32))
        assert np.array_equal(bits(out[s]), bits(want))
        assert np.array_equal(dev[s].cpu().numpy(), colour[s])
    # max_samples and min_scale reach the library
    capped = model.warped_crops_tensor((24, 20), filter="area", max_samples=2, min_scale=1.5, **kw)
    assert np.array_equal(capped[3], want_samples(mats, flags, align_filter("area", 2, 1.5))) and capped[3].max() == 2
    after = (c.get_x(), tr.get(ids), model.aligned_crops_tensor(16, lm, dtype="uint8"))      # the crop source is the context's images again
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(bits(before[1][0]), bits(after[1][0])) and np.array_equal(before[1][1], after[1][1])
    for p, q in zip(before[2], after[2]):
        assert np.array_equal(bits(p), bits(q))
    c.close()


def test_behind_tracker_step_and_detect_batch(built):
    import torch
    model = random_model()
    frames, _, boxes = synth.make_tracks(2, 2, seed=58)
    ids = np.arange(2)
    tr = model.tracker(2)
    tr.start(ids, boxes[0])
    c = model.optimised_model.ctx
    kw = dict(dtype="float32", channels=1, filter="area")
    for step in range(2):
        dev = [torch.from_numpy(f).cuda() for f in frames[step]]
        rows, lost = tr.step(ids, dev)
        a = model.warped_crops_tensor(24, **kw)
        assert len(a) == 4 and np.array_equal(bits(c.get_x()), bits(rows))
        c.set_x(c.get_x())
        b = model.warped_crops_tensor(24, **kw)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
        assert np.isfinite(a[1]).all() and a[0].cpu().numpy().any()
    rows = model.detect_batch(list(frames[1]), boxes[1])
    a = model.warped_crops_tensor((33, 17), **kw)
    c = model.optimised_model.ctx
    assert len(a) == 4 and np.array_equal(bits(c.get_x()), bits(rows))
    lab = c.warp_labels()
    want_s = want_samples(a[1], a[2], AREA)
    assert np.array_equal(a[3], want_s) and (want_s > 1).any()
    for s in range(2):
        want = WA.tensor(T.Frame(T.GRAY, frames[1][s]), a[1][s].reshape(-1, 6), lab, want_s[s], dtype="float32", channels=1)
        assert np.array_equal(bits(a[0][s]), bits(want))
    c.close()
