"""Aligned crops as network input tensors on the device (csrc/sdm_align_tensor.hip, include/sdm.h sdm_align_crops_tensor and
sdm_align_set_source_frames, detection_model.aligned_crops_tensor).  State comes from set_model_geometry and set_x; every comparison
of crop elements is bit for bit against the host restatement (tests/align_tensor_ref.py) applied to the device's own M."""
import itertools

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
from superviseddescent_amd import Context, HoGParam, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, ibug, synth

pytestmark = pytest.mark.gpu
IDS = ibug.RCR22_IDS
L = len(IDS)
RE, LE = ibug.eye_indices(IDS)
MEAN = ibug.select_mean(IDS)
PARAMS = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
LM = np.array([3, 6, 9, 12, 15])
SCALE, BIAS = np.float32(1 / 58.395), np.float32(-2.1179)
SCALES = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], np.float32)
BIASES = np.array([-2.1179, -2.0357, -1.8044], np.float32)
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))


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


def code(fn, *a, **k):
    with pytest.raises(SdmError) as e:
        fn(*a, **k)
    return e.value.code


def device_frames(buf, frames):
    """(the buffer on the device, the frame list Context.set_frames_device takes, the chroma pointers): views into the one buffer"""
    import torch
    dev = torch.from_numpy(buf).cuda()
    base = dev.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["stride"], K.NAMES[f["fmt"]]) for f in frames]
    chroma = [base + f["uv_off"] if f["fmt"] == T.NV12 and f.get("separate") else None for f in frames]
    return dev, lst, chroma


def install(ctx, buf, frames, idx, w, h, seed):
    """frames as the context's images and as the crop source; rows from known similarities; returns what must stay alive"""
    dev, lst, chroma = device_frames(buf, frames)
    ctx.set_frames_device(lst)
    ctx.set_sample_image_index(idx)
    x = K.landmark_rows(K.similarities(frames, idx, w, h, seed), template(w, h), LM, L)
    ctx.set_x(x)
    ctx.align_set_source_frames(lst, chroma=chroma)
    return dev, lst, chroma, x


def check_call(ctx, host, idx, w, h, cache, **spec):
    """one call against the restatement; cache: the warped pixels per row (they do not depend on the spec)"""
    out, mats, flags = ctx.align_crops_tensor(LM, template(w, h), w, h, **spec)
    got = out.cpu().numpy()
    for r, im in enumerate(idx):
        if r not in cache:
            kind, bgr = T.warped(host[im], mats[r], w, h)
            cache[r] = (mats[r].copy(), kind, bgr, T.luma(host[im], mats[r], w, h) if kind == "nv12" else None,
                        A.PARTIAL if A.partial(mats[r], w, h, host[im].w, host[im].h) else 0)
        m, kind, bgr, y, flag = cache[r]
        assert np.array_equal(bits(m), bits(mats[r])) and flags[r] == flag, r
        want = T.finish(kind, bgr, y, **spec)
        assert got[r].dtype == want.dtype and got[r].shape == want.shape
        assert np.array_equal(bits(got[r]), bits(want)), (r, host[im].fmt, spec)
    return out, mats, flags


def test_existing_path_is_the_special_case(ctx):
    import torch
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (29, 37), dtype=np.uint8), rng.integers(0, 256, (48, 64), dtype=np.uint8)]
    frames = [dict(w=37, h=29), dict(w=64, h=48)]
    idx = [0, 1, 1, 0]
    ctx.upload_images(imgs)
    ctx.set_sample_image_index(idx)
    for (w, h) in K.CROPS:
        ctx.set_x(K.landmark_rows(K.similarities(frames, idx, w, h, 5), template(w, h), LM, L))
        ctx.align_set_source(None)
        crops, mats, flags = ctx.align_crops(LM, template(w, h), w, h)
        out, m2, f2 = ctx.align_crops_tensor(LM, template(w, h), w, h, dtype="uint8", layout="nhwc", channels=1)
        assert np.array_equal(out.cpu().numpy(), crops) and np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
        assert flags.any()
    # a BGR stack of equally sized images
    stack = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    ctx.upload_images([imgs[1], imgs[1]])
    frames = [dict(w=64, h=48)] * 2
    for src in (stack, torch.from_numpy(stack).cuda()):
        assert ctx.align_set_source(src) == 3
        for (w, h) in K.CROPS:
            ctx.set_x(K.landmark_rows(K.similarities(frames, idx, w, h, 6), template(w, h), LM, L))
            crops, mats, _ = ctx.align_crops(LM, template(w, h), w, h)
            out, m2, _ = ctx.align_crops_tensor(LM, template(w, h), w, h, dtype="uint8", layout="nhwc", channels=3, order="bgr")
            assert np.array_equal(out.cpu().numpy(), crops) and np.array_equal(bits(m2), bits(mats))
    ctx.align_set_source(None)
    ctx.set_sample_image_index(None)


def test_ragged_frame_list_all_formats_in_one_call(ctx):
    buf, frames = K.place(K.RAGGED, 11)
    host = [K.host_frame(buf, f) for f in frames]
    idx = [5, 3, 1, 0, 2, 4]
    seen = 0
    for (w, h) in K.CROPS:
        keep = install(ctx, buf, frames, idx, w, h, 30 + w)
        cache = {}
        for dtype, layout, channels, order in COMBOS:
            _, _, flags = check_call(ctx, host, idx, w, h, cache, dtype=dtype, layout=layout, channels=channels, order=order,
                                     scale=SCALES, bias=BIASES, gray_shift=14 if order == "bgr" else 15)
            seen |= int(flags.max())
        assert np.array_equal(keep[0].cpu().numpy(), buf)                 # the in-place source is only read
    assert seen & A.PARTIAL
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_nv12(ctx):
    buf, frames = K.place(K.NV12, 12)
    host = [K.host_frame(buf, f) for f in frames]
    idx = [0, 1, 2, 3]
    for (w, h) in K.CROPS:
        dev, lst, chroma, x = install(ctx, buf, frames, idx, w, h, 40 + w)
        cache = {}
        for layout, order in (("nchw", "rgb"), ("nhwc", "bgr")):
            check_call(ctx, host, idx, w, h, cache, dtype="uint8", layout=layout, channels=3, order=order)
            check_call(ctx, host, idx, w, h, cache, dtype="float16", layout=layout, channels=3, order=order, scale=SCALE, bias=BIAS)
        y1, mats, _ = check_call(ctx, host, idx, w, h, cache, dtype="uint8", layout="nhwc", channels=1)
        # one channel: the bits of sdm_align_crops on the same luma (the context's images ARE the Y planes)
        ctx.align_set_source(None)
        crops, m2, _ = ctx.align_crops(LM, template(w, h), w, h)
        assert np.array_equal(y1.cpu().numpy(), crops) and np.array_equal(bits(mats), bits(m2))
    # neutral chroma gives R = G = B
    flat = buf.copy()
    for f in frames:
        flat[f["uv_off"]:f["uv_off"] + K.plane_bytes(f)[1]] = 128
    dev, lst, chroma, x = install(ctx, flat, frames, idx, 16, 16, 47)
    out, _, _ = ctx.align_crops_tensor(LM, template(16, 16), 16, 16, dtype="uint8", layout="nhwc", channels=3)
    got = out.cpu().numpy()
    assert got.any() and np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 1], got[..., 2])
    # a crop wholly outside the frame: (0, 0, 0) before scale and bias
    far = x.copy()
    far[0, :L] += 500.0
    ctx.set_x(far)
    out, _, flags = ctx.align_crops_tensor(LM, template(16, 16), 16, 16, dtype="float32", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    got = out.cpu().numpy()
    assert flags[0] == A.PARTIAL
    for c in range(3):
        assert np.array_equal(bits(got[0, c]), bits(np.full((16, 16), T.element(0, SCALES[c], BIASES[c], "float32"))))
    ctx.align_set_source_frames(None)


def test_element_formula_on_device(ctx):
    import torch
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ctx.upload_images([img])
    ctx.set_sample_image_index(None)
    t = template(16, 16)
    x = K.landmark_rows([A.similarity(1, 0, 0, 0)], t, LM, L)            # the row's landmarks ARE the template: identity
    ctx.set_x(x)
    ctx.align_set_source(None)
    for dtype in ("float32", "float16"):
        out, mats, flags = ctx.align_crops_tensor(LM, t, 16, 16, dtype=dtype, layout="nchw", channels=1, scale=SCALE, bias=BIAS)
        assert np.array_equal(mats[0], np.array([[1, 0, 0], [0, 1, 0]], np.float32)) and flags[0] == 0
        assert np.array_equal(bits(out[0, 0]), bits(T.element(img, SCALE, BIAS, dtype)))
    u8, _, _ = ctx.align_crops_tensor(LM, t, 16, 16, dtype="uint8", channels=1)
    assert np.array_equal(u8.cpu().numpy()[0, 0], img)
    dev = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device="cuda")
    got, _, _ = ctx.align_crops_tensor(LM, t, 16, 16, out=dev, scale=SCALES, bias=BIASES)
    assert got is dev
    for c in range(3):
        assert np.array_equal(bits(dev[0, c]), bits(T.element(img, SCALES[c], BIASES[c], "float16")))


def test_degenerate_row(ctx):
    buf, frames = K.place(K.RAGGED, 11)
    idx = [0, 1, 2, 4]
    dev, lst, chroma, x = install(ctx, buf, frames, idx, 7, 7, 55)
    spec = dict(dtype="float32", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    clean, m0, f0 = ctx.align_crops_tensor(LM, template(7, 7), 7, 7, **spec)
    bad = x.copy()
    bad[1, LM[2]] = np.nan
    ctx.set_x(bad)
    for dtype in ("float32", "float16", "uint8"):
        out, mats, flags = ctx.align_crops_tensor(LM, template(7, 7), 7, 7, **dict(spec, dtype=dtype))
        got = out.cpu().numpy()
        assert flags[1] == A.DEGENERATE and np.isnan(mats[1]).all()
        for c in range(3):
            assert np.array_equal(bits(got[1, c]), bits(np.full((7, 7), T.element(0, SCALES[c], BIASES[c], dtype))))
        if dtype == "float32":
            keep = [0, 2, 3]
            assert np.array_equal(bits(got[keep]), bits(clean[keep])) and np.array_equal(bits(mats[keep]), bits(m0[keep]))
            assert np.array_equal(flags[keep], f0[keep])
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_rows_are_independent(ctx):
    buf, frames = K.place(K.RAGGED, 11)
    n = 257
    idx = (np.arange(n) * 5 + 1) % 6
    dev, lst, chroma, x = install(ctx, buf, frames, idx, 7, 7, 60)
    spec = dict(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    out, mats, flags = ctx.align_crops_tensor(LM, template(7, 7), 7, 7, **spec)
    got = out.cpu().numpy()
    for r in (0, 1, 2, 63, 64, 128, 255, 256):
        ctx.set_sample_image_index(idx[r:r + 1])
        ctx.set_x(x[r:r + 1])
        one, m1, f1 = ctx.align_crops_tensor(LM, template(7, 7), 7, 7, **spec)
        assert np.array_equal(bits(one[0]), bits(got[r])) and np.array_equal(bits(m1[0]), bits(mats[r])) and f1[0] == flags[r]
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def test_tracker_hand_off(built):
    import torch
    rng = np.random.default_rng(77)
    R = [rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32) for p in PARAMS]
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, r in zip(regs, R):
        reg.x = r
    model = detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS)
    frames, _, boxes = synth.make_tracks(2, 3, seed=58)                     # frames x streams x H x W
    cut = ((slice(0, 230), slice(0, 256)), (slice(0, 256), slice(0, 241)))
    colour = []
    for t in range(3):
        row = []
        for s in range(2):
            g = frames[t, s][cut[s]]
            c = rng.integers(0, 256, g.shape + (3,), dtype=np.uint8)
            c[..., 1] = g
            row.append(c)
        colour.append(row)
    ids = np.arange(2)

    def run(with_crops):
        tr = model.tracker(2)
        tr.start(ids, boxes[0])
        res = []
        for t in range(3):
            dev = [torch.from_numpy(c).cuda() for c in colour[t]]
            rows, lost = tr.step(ids, dev)
            if with_crops:
                out, mats, flags = model.aligned_crops_tensor(16, [IDS[i] for i in LM], frames=dev, mean=[123.675, 116.28, 103.53],
                                                              std=[58.395, 57.12, 57.375])
                assert tuple(out.shape) == (2, 3, 16, 16) and out.dtype == torch.float16
                spec = _lib.align_tensor_spec(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
                for s in range(2):
                    want = T.tensor(T.Frame(T.BGR, colour[t][s]), mats[s], 16, 16, scale=np.array(spec.scale, np.float32),
                                    bias=np.array(spec.bias, np.float32))
                    assert np.array_equal(bits(out[s]), bits(want))
                    assert np.array_equal(dev[s].cpu().numpy(), colour[t][s])        # the in-place source is unchanged
            res.append((rows, lost, tr.get(ids)))
        return res

    a, b = run(True), run(False)
    for (r1, l1, (x1, s1)), (r2, l2, (x2, s2)) in zip(a, b):
        assert np.array_equal(bits(r1), bits(r2)) and np.array_equal(l1, l2) and np.array_equal(bits(x1), bits(x2)) and np.array_equal(s1, s2)
    model.optimised_model.ctx.close()


def test_refusals(ctx):
    import ctypes
    import torch
    buf, frames = K.place(K.RAGGED, 11)
    idx = [0, 1, 3, 4, 5]
    dev, lst, chroma, x = install(ctx, buf, frames, idx, 16, 16, 70)
    t = template(16, 16)
    spec = dict(dtype="float16", layout="nchw", channels=3, scale=SCALES, bias=BIASES)
    good = ctx.align_crops_tensor(LM, t, 16, 16, **spec)

    def same():
        now = ctx.align_crops_tensor(LM, t, 16, 16, **spec)
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(now, good))

    lib, h = ctx._lib, ctx._h
    out = torch.zeros((5, 3, 16, 16), dtype=torch.float16, device="cuda")
    mis = torch.zeros(5 * 3 * 16 * 16 + 4, dtype=torch.float16, device="cuda")[4:].view(5, 3, 16, 16)       # 8 bytes off
    idx32, t32 = np.ascontiguousarray(LM, np.int32), np.ascontiguousarray(t)

    def raw(spec_ptr, out_ptr, k=LM.size, w=16, hh=16, lm=idx32, tm=t32):
        rc = lib.sdm_align_crops_tensor(h, lm.ctypes.data, tm.ctypes.data, k, w, hh, spec_ptr, ctypes.c_void_p(out_ptr), None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def S(**kw):
        s = _lib.align_tensor_spec(**dict(spec, **{k: v for k, v in kw.items() if k in ("scale", "bias")}))
        for k, v in kw.items():
            if k not in ("scale", "bias"):
                setattr(s, k, v)
        return ctypes.byref(s)

    nan3, inf3 = [1, np.nan, 1], [0, 0, np.inf]
    cases = [
        lambda: raw(None, out.data_ptr()),                                         # spec NULL
        lambda: raw(S(dtype=3), out.data_ptr()), lambda: raw(S(dtype=-1), out.data_ptr()),
        lambda: raw(S(layout=2), out.data_ptr()), lambda: raw(S(order=2), out.data_ptr()),
        lambda: raw(S(channels=2), out.data_ptr()), lambda: raw(S(channels=4), out.data_ptr()), lambda: raw(S(channels=0), out.data_ptr()),
        lambda: raw(S(gray_shift=13), out.data_ptr()), lambda: raw(S(gray_shift=16), out.data_ptr()),
        lambda: raw(S(scale=nan3), out.data_ptr()), lambda: raw(S(bias=inf3), out.data_ptr()),
        lambda: raw(S(), 0), lambda: raw(S(), mis.data_ptr()),                     # out NULL, misaligned
        # everything sdm_align_crops refuses
        lambda: raw(S(), out.data_ptr(), k=1), lambda: raw(S(), out.data_ptr(), k=L + 1),
        lambda: raw(S(), out.data_ptr(), lm=np.array([3, 3, 9, 12, 15], np.int32)), lambda: raw(S(), out.data_ptr(), lm=np.array([3, L, 9, 12, 15], np.int32)),
        lambda: raw(S(), out.data_ptr(), tm=np.full_like(t32, 2.0)), lambda: raw(S(), out.data_ptr(), tm=np.where(np.arange(5)[:, None] == 1, np.nan, t32).astype(np.float32)),
        lambda: raw(S(), out.data_ptr(), w=0), lambda: raw(S(), out.data_ptr(), hh=1025),
        lambda: lib.sdm_align_crops_tensor(h, None, t32.ctypes.data, 5, 16, 16, S(), ctypes.c_void_p(out.data_ptr()), None, None) and _raise(lib),
    ]
    for f in cases:
        assert code(f) == -1
        assert same()
    raw(S(dtype=_lib.SDM_ALIGN_U8, scale=nan3), torch.zeros((5, 3, 16, 16), dtype=torch.uint8, device="cuda").data_ptr())   # ignored for U8
    # sdm_align_set_source_frames: what sdm_set_frames_device refuses of a frame, and a short NV12 stride
    p = dev.data_ptr()
    bad_lists = [[(p, 0, 4, 16, "gray")], [(p, 4, 0, 16, "gray")], [(0, 4, 4, 16, "gray")], [(p, 4, 4, 11, "bgr")], [(p, 4, 4, 15, "rgba")],
                 [(p, 4, 4, 16, 6)], [(p, 4, 4, 16, -1)], [(p, 5, 4, 5, "nv12")], [(p, 4, 4, 3, "nv12")], lst[:2] + [(p, 4, 4, 3, "gray")]]
    for bl in bad_lists:
        assert code(ctx.align_set_source_frames, bl) == -1
        assert same()
    arr = (_lib.SdmFrame * 1)(_lib.SdmFrame(p, 4, 4, 16, 0))
    assert lib.sdm_align_set_source_frames(h, arr, None, -1) == -1 and same()
    # sources that do not cover the rows: a list that is too short, a frame of another size
    ctx.align_set_source_frames(lst[:5], chroma=chroma[:5])
    assert code(ctx.align_crops_tensor, LM, t, 16, 16, **spec) == -1
    wrong = list(lst)
    wrong[1] = (lst[1][0], lst[1][1] - 1, lst[1][2], lst[1][3], lst[1][4])
    ctx.align_set_source_frames(wrong, chroma=chroma)
    assert code(ctx.align_crops_tensor, LM, t, 16, 16, **spec) == -1
    # sdm_align_crops on an NV12 / mixed list is refused and names the tensor call; on a list of one pixel size it works
    ctx.align_set_source_frames(lst, chroma=chroma)
    with pytest.raises(SdmError, match="sdm_align_crops_tensor"):
        ctx.align_crops(LM, t, 16, 16)
    assert same()
    assert ctx.align_set_source_frames([lst[2]] * 6) is None                         # NV12 alone
    with pytest.raises(SdmError, match="sdm_align_crops_tensor"):
        ctx.align_crops(LM, t, 16, 16)
    ctx.align_set_source_frames(lst, chroma=chroma)
    assert same()
    fresh = Context(0)
    try:
        assert code(fresh.align_crops_tensor, LM, t, 16, 16, **spec) == -1               # no geometry, no rows
    finally:
        fresh.close()
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def _raise(lib):
    raise SdmError(-1, lib.sdm_last_error().decode())


def test_source_replacement_and_uniform_lists(ctx):
    import torch
    rng = np.random.default_rng(90)
    n, w, h = 3, 16, 16
    gray = rng.integers(0, 256, (n, 20, 24), dtype=np.uint8)
    stack = torch.from_numpy(rng.integers(0, 256, (n, 20, 24, 3), dtype=np.uint8)).cuda()
    rgba = [torch.from_numpy(rng.integers(0, 256, (20, 24, 4), dtype=np.uint8)).cuda() for _ in range(n)]
    ctx.upload_images(list(gray))
    ctx.set_sample_image_index(None)
    frames = [dict(w=24, h=20)] * n
    ctx.set_x(K.landmark_rows(K.similarities(frames, range(n), w, h, 91), template(w, h), LM, L))
    t = template(w, h)
    spec = dict(dtype="float32", layout="nhwc", channels=3, order="bgr", scale=SCALES, bias=BIASES)
    setters = {"stack": lambda: ctx.align_set_source(stack), "list": lambda: ctx.align_set_source_frames(rgba, "rgba"),
               "none": lambda: ctx.align_set_source(None), "none2": lambda: ctx.align_set_source_frames(None)}
    hosts = {"stack": [T.Frame(T.BGR, s) for s in stack.cpu().numpy()], "list": [T.Frame(T.RGBA, f.cpu().numpy()) for f in rgba],
             "none": [T.Frame(T.GRAY, g) for g in gray]}
    hosts["none2"] = hosts["none"]
    for order in itertools.permutations(("stack", "list", "none")):
        for name in order + ("none2", "list", "stack"):
            setters[name]()
            out, mats, _ = ctx.align_crops_tensor(LM, t, w, h, **spec)
            for r in range(n):
                assert np.array_equal(bits(out[r]), bits(T.tensor(hosts[name][r], mats[r], w, h, **spec))), (order, name, r)
    # sdm_align_crops on a list of one pixel size: the interleaved warp of a stack, alpha included
    assert ctx.align_set_source_frames(rgba, "rgba") == 4
    crops, mats, _ = ctx.align_crops(LM, t, w, h)
    assert crops.shape == (n, h, w, 4)
    for r in range(n):
        assert np.array_equal(crops[r], A.warp(rgba[r].cpu().numpy(), mats[r], w, h))
    ctx.align_set_source(None)
    assert ctx.align_crops(LM, t, w, h)[0].shape == (n, h, w, 1)
