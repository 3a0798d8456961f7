"""Area-averaged crop tensors on the device (csrc/sdm_align_area.hip, include/sdm.h sdm_align_crops_tensor_filtered,
Context.align_crops_tensor(filter=...)).  State comes from set_model_geometry and set_x; every comparison of crop elements is bit for
bit against the host restatement (tests/align_area_ref.py) applied to the device's own M.

No frame set here has a plane beyond INT_MAX bytes (tests/frame_geometry_cases.py builds its own in a 4.5 GiB buffer): the 64-bit offset
path of the sub-sample loop is covered by the host build, tests/test_align_area_host.py."""
import ctypes
import itertools

import numpy as np
import pytest

import align_area_cases as C
import align_area_ref as R
import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
from superviseddescent_amd import Context, HoGParam, SdmError, _lib, ibug

pytestmark = pytest.mark.gpu
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
LM = C.LM
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
assert L == C.L


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def template(w, h):
    """K points spread over the crop (crop pixels)"""
    return (np.array([[0.2, 0.2], [0.8, 0.25], [0.5, 0.5], [0.3, 0.8], [0.75, 0.7]]) * (w - 1 + 1e-3, h - 1 + 1e-3)).astype(np.float32) + 0.125


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def install(ctx, buf, frames, idx, sims, w, h):
    """frames as the context's images and as the crop source; rows from the similarities; returns what must stay alive"""
    import torch
    dev = torch.from_numpy(buf).cuda()
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], K.NAMES[f["fmt"]]) for f in frames]
    chroma = [base + f["uv_off"] if f["fmt"] == T.NV12 and f.get("separate") else None for f in frames]
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    ctx.set_x(K.landmark_rows(sims, template(w, h), LM, L))
    ctx.align_set_source_frames(lst, chroma=chroma)
    return dev


def check_set(ctx, specs, seed, combos):
    """every frame of the set at S = 1, 2, 3, 5 and 16, calls of 10 rows that each mix the five, all `combos` on every call"""
    buf, frames = K.place(specs, seed)
    host = [K.host_frame(buf, f) for f in frames]
    seen, partial = set(), 0
    for (w, h) in K.CROPS:
        for idx, sims, want_S in C.mixed_rows(frames, w, h, seed + w):
            keep = install(ctx, buf, frames, idx, sims, w, h)
            t = template(w, h)
            _, m0, f0 = ctx.align_crops_tensor(LM, t, w, h, dtype="uint8", channels=1)
            cache = None
            for dtype, layout, channels, order in combos:
                spec = dict(dtype=dtype, layout=layout, channels=channels, order=order, scale=SCALES, bias=BIASES,
                            gray_shift=14 if order == "bgr" else 15)
                out, mats, flags, samples = ctx.align_crops_tensor(LM, t, w, h, filter="area", **spec)
                # M and the flags are sdm_align_crops_tensor's; S is the rule's on the device's M
                assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
                assert samples.dtype == np.int32 and list(samples) == want_S
                assert list(samples) == [R.samples(m) for m in mats]
                if cache is None:
                    cache = [R.warped(host[im], mats[r], w, h, int(samples[r])) for r, im in enumerate(idx)]
                got = out.cpu().numpy()
                for r, im in enumerate(idx):
                    want = T.finish(*cache[r], **spec)
                    assert got[r].dtype == want.dtype and got[r].shape == want.shape
                    assert np.array_equal(bits(got[r]), bits(want)), (r, host[im].fmt, int(samples[r]), spec)
                    seen.add((host[im].fmt, int(samples[r])))
            partial |= int(f0.max())
            assert np.array_equal(keep.cpu().numpy(), buf)                # the in-place source is only read
    assert seen == {(f.fmt, S) for f in host for _, S in C.CLASSES}       # every format at every S
    assert partial & A.PARTIAL                                            # footprints hang over the frames' edges
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_ragged_frame_list_all_formats_at_every_s(ctx):
    check_set(ctx, K.RAGGED, 11, COMBOS)


def test_nv12_at_every_s(ctx):
    check_set(ctx, K.NV12, 12, COMBOS)


def test_old_path_preserved(ctx):
    buf, frames = K.place(K.RAGGED, 11)
    w, h = 16, 16
    idx, sims, want_S = C.mixed_rows(frames, w, h, 77)[0]
    keep = install(ctx, buf, frames, idx, sims, w, h)
    t = template(w, h)
    assert max(want_S) == 16
    for dtype, layout, channels in (("float16", "nchw", 3), ("uint8", "nhwc", 3), ("float32", "nchw", 1)):
        spec = dict(dtype=dtype, layout=layout, channels=channels, scale=SCALES, bias=BIASES)
        plain, m0, f0 = ctx.align_crops_tensor(LM, t, w, h, **spec)
        area = ctx.align_crops_tensor(LM, t, w, h, filter="area", **spec)
        assert list(area[3]) == want_S and not np.array_equal(bits(area[0]), bits(plain))
        for filt in (_lib.align_filter("bilinear"), _lib.align_filter("area", max_samples=1), _lib.align_filter("area", min_scale=1e6),
                     _lib.align_filter("area", min_scale=1e30), "bilinear"):
            out, mats, flags, samples = ctx.align_crops_tensor(LM, t, w, h, filter=filt, **spec)
            assert np.array_equal(bits(out), bits(plain)) and np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0)
            assert np.all(samples == 1)
        # the rows with S = 1 of a mixed call have the old call's bits as well
        ones = np.array(want_S) == 1
        assert ones.any() and np.array_equal(bits(area[0])[ones], bits(plain)[ones])
    assert np.array_equal(keep.cpu().numpy(), buf)
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_sub_sample_beyond_2_20_zeroes_the_pixel(ctx):
    """column 3 of the crop has its centre at sx = 2^20 exactly (accepted) and its right sub-samples at 2^20 + 0.5 (refused)"""
    w, h, tx, ty = 5, 3, 2 ** 20 - 6, 1
    img = np.full((8, 2 ** 20 + 8), 255, np.uint8)
    tmpl = np.array([[0, 0], [4, 0], [2, 1], [0, 2], [4, 2]], np.float32)
    x = np.zeros((1, 2 * L), np.float32)
    x[0, LM], x[0, L + LM] = 2 * tmpl[:, 0] + tx, 2 * tmpl[:, 1] + ty
    ctx.upload_images([img])
    ctx.set_sample_image_index(None)
    ctx.set_x(x)
    ctx.align_set_source(None)
    plain, m0, f0 = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", layout="nhwc", channels=1)
    out, mats, flags, samples = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", layout="nhwc", channels=1, filter="area")
    assert np.array_equal(mats[0], np.array([[2, 0, tx], [0, 2, ty]], np.float32)) and samples[0] == 2 and flags[0] == f0[0]
    got, old = out.cpu().numpy()[0, :, :, 0], plain.cpu().numpy()[0, :, :, 0]
    assert np.all(got[:, :3] == 255) and np.all(got[:, 3:] == 0)
    assert np.all(old[:, :4] == 255) and np.all(old[:, 4] == 0)           # bilinear: the centre of column 3 is accepted
    _, bgr, _ = R.warped(T.Frame(T.GRAY, img), mats[0], w, h, 2)
    assert np.array_equal(got, bgr[..., 0])
    f32out, _, _, _ = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="float32", channels=3, scale=SCALES, bias=BIASES, filter="area")
    for c in range(3):
        assert np.array_equal(bits(f32out[0, c, :, 3:]), bits(np.full((h, 2), T.element(0, SCALES[c], BIASES[c], "float32"))))


def test_degenerate_row(ctx):
    buf, frames = K.place(K.RAGGED, 11)
    w, h = 7, 7
    idx, sims, want_S = C.mixed_rows(frames, w, h, 55)[1]
    keep_alive = install(ctx, buf, frames, idx, sims, w, h)
    x = K.landmark_rows(sims, template(w, h), LM, L)
    spec = dict(layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    bad_row = int(np.argmax(np.array(want_S) == 16))
    clean = ctx.align_crops_tensor(LM, template(w, h), w, h, dtype="float32", filter="area", **spec)
    assert clean[3][bad_row] == 16
    bad = x.copy()
    bad[bad_row, LM[2]] = np.nan
    ctx.set_x(bad)
    for dtype in ("float32", "float16", "uint8"):
        out, mats, flags, samples = ctx.align_crops_tensor(LM, template(w, h), w, h, dtype=dtype, filter="area", **spec)
        got = out.cpu().numpy()
        assert flags[bad_row] == A.DEGENERATE and np.isnan(mats[bad_row]).all() and samples[bad_row] == 1
        for c in range(3):
            assert np.array_equal(bits(got[bad_row, c]), bits(np.full((h, w), T.element(0, SCALES[c], BIASES[c], dtype))))
        if dtype == "float32":
            keep = np.arange(len(idx)) != bad_row
            assert np.array_equal(bits(got[keep]), bits(clean[0])[keep]) and np.array_equal(samples[keep], clean[3][keep])
    assert np.array_equal(keep_alive.cpu().numpy(), buf)
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_refusals(ctx):
    import torch
    buf, frames = K.place(K.RAGGED, 11)
    w, h = 16, 16
    idx, sims, _ = C.mixed_rows(frames, w, h, 70)[0]
    keep_alive = install(ctx, buf, frames, idx, sims, w, h)
    t = np.ascontiguousarray(template(w, h))
    lm = np.ascontiguousarray(LM, np.int32)
    n = len(idx)
    spec = _lib.align_tensor_spec(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    out = torch.full((n, 3, h, w), 7.0, dtype=torch.float16, device="cuda")
    mis = torch.zeros(n * 3 * h * w + 4, dtype=torch.float16, device="cuda")[4:].view(n, 3, h, w)        # 8 bytes off
    lib, hd = ctx._lib, ctx._h

    def raw(filt, spec_ptr=ctypes.byref(spec), out_ptr=out.data_ptr(), k=LM.size, ww=w):
        return lib.sdm_align_crops_tensor_filtered(hd, lm.ctypes.data, t.ctypes.data, k, ww, h, spec_ptr, filt, ctypes.c_void_p(out_ptr),
                                                   None, None, None)

    F = lambda mode=1, cap=16, gate=1.0: ctypes.byref(_lib.SdmAlignFilter(mode, cap, gate))
    bad_spec = _lib.align_tensor_spec(dtype="float16")
    bad_spec.channels = 2
    cases = [lambda: raw(None), lambda: raw(F(mode=2)), lambda: raw(F(mode=-1)), lambda: raw(F(cap=0)), lambda: raw(F(cap=17)),
             lambda: raw(F(cap=-3)), lambda: raw(F(gate=0.5)), lambda: raw(F(gate=float("nan"))), lambda: raw(F(gate=float("inf"))),
             lambda: raw(F(gate=-2.0)),
             # what sdm_align_crops_tensor refuses
             lambda: raw(F(), spec_ptr=None), lambda: raw(F(), spec_ptr=ctypes.byref(bad_spec)), lambda: raw(F(), out_ptr=0),
             lambda: raw(F(), out_ptr=mis.data_ptr()), lambda: raw(F(), k=1), lambda: raw(F(), ww=1025)]
    for f in cases:
        assert f() == -1 and lib.sdm_last_error()
        assert bool((out == 7.0).all())                                   # nothing was launched
    assert raw(F()) == 0 and not bool((out == 7.0).all())
    # the Python layer
    for bad in ("box", 3, _lib.align_tensor_spec()):
        with pytest.raises(ValueError):
            ctx.align_crops_tensor(LM, t, w, h, filter=bad)
    with pytest.raises(SdmError):
        ctx.align_crops_tensor(LM, t, w, h, filter=_lib.SdmAlignFilter(1, 17, 1.0))
    assert np.array_equal(keep_alive.cpu().numpy(), buf)
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


@pytest.mark.parametrize("scale", [4, 8])
def test_stripes_on_the_device(ctx, scale):
    frame, x, tmpl, w, h, M_want = C.stripes(scale)
    ctx.upload_images([frame])
    ctx.set_sample_image_index(None)
    ctx.set_x(x)
    ctx.align_set_source(None)
    plain, _, _ = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", channels=1)
    out, mats, flags, samples = ctx.align_crops_tensor(LM, tmpl, w, h, dtype="uint8", channels=1, filter="area")
    assert np.array_equal(mats[0], M_want.astype(np.float32)) and flags[0] == 0 and samples[0] == scale
    assert bool((out == 128).all())                                       # every footprint lies inside the frame
    assert set(np.unique(plain.cpu().numpy())) <= {0, 255}


def test_model_layer_returns_samples(built):
    """detection_model.aligned_crops_tensor(filter=...): the 4-tuple with a filter, the old 3-tuple without"""
    import torch
    from superviseddescent_amd import LinearRegressor, SupervisedDescentOptimiser, detection_model
    rng = np.random.default_rng(3)
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, p in zip(regs, PARAMS):
        reg.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32)
    model = detection_model(SupervisedDescentOptimiser(regs), ibug.select_mean(IDS), IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    c = model.optimised_model.ctx
    c.set_model_geometry(L, RE, LE, PARAMS)
    frame = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    dev = torch.from_numpy(frame).cuda()
    c.set_frames_device([dev], "bgr")
    c.set_sample_image_index(None)
    ids = [IDS[i] for i in LM]
    t = template(16, 16)
    sim = A.similarity(4.5, 10.0, 20.0, 8.0)
    c.set_x(K.landmark_rows([sim], t, LM, L))
    old = model.aligned_crops_tensor(16, ids, template=t, frames=[dev], formats="bgr")
    assert len(old) == 3
    for filt in ("area", _lib.align_filter("area", 16, 1.0)):
        out, mats, flags, samples = model.aligned_crops_tensor(16, ids, template=t, frames=[dev], formats="bgr", filter=filt)
        assert samples[0] == 5 and np.array_equal(bits(mats), bits(old[1]))
        want = R.tensor(T.Frame(T.BGR, frame), mats[0], 16, 16, 5)
        assert np.array_equal(bits(out[0]), bits(want))
    c.close()
