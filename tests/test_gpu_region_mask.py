"""Landmark region masks on the device (csrc/sdm_region_mask.hip, include/sdm.h "Landmark region masks", Context.align_region_mask[_at],
detection_model.region_masks).  Every comparison is bit for bit against the numpy restatement (tests/region_mask_ref.py) and on the
WHOLE output buffer: the maps and 64 guard bytes of noise before and after them."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import paste_ref as P
import region_mask_cases as C
import region_mask_ref as R
from test_gpu_align_tensor import IDS, L, LE, LM, MEAN, PARAMS, RE, bits, code, install, template
from test_region_mask_host import FLAGGED
from superviseddescent_amd import Context, LinearRegressor, SdmError, SupervisedDescentOptimiser, _lib, detection_model, ibug

pytestmark = pytest.mark.gpu
f32 = np.float32
OUTLINE = ("outline_hole", [27, 12], 1, 0)


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    c.set_model_geometry(L, RE, LE, PARAMS)
    yield c
    c.close()


def hull_list(bits_, n):
    return [g for g in range(n) if bits_ >> g & 1]


def guarded_out(n, w, h, seed=7):
    """(the noise buffer on the device, its host copy, the N x h x w view 64 bytes in)"""
    import torch
    host, inner = C.guarded(n * w * h, seed)
    dev = torch.from_numpy(host.copy()).cuda()
    return dev, host, dev[inner].view(n, h, w)


def draw_at(ctx, rows, sizes, nh, bits_, w, h, grow, feather):
    """one _at call on guarded output: (the whole buffer back on the host, the noise it started as, flags)"""
    dev, host, view = guarded_out(len(rows), w, h)
    mats = np.stack([M for M, _ in rows])
    pts = np.stack([p for _, p in rows])
    out, flags = ctx.align_region_mask_at(mats, pts, w, h, sizes, nh, hull_list(bits_, len(sizes)), grow, feather, out=view)
    assert out.data_ptr() == view.data_ptr()
    return dev.cpu().numpy(), host, flags


def with_maps(host, maps):
    want = host.copy()
    want[64:64 + maps.size] = maps.reshape(-1)
    return want


@pytest.mark.parametrize("crop", C.CROPS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_shapes_and_parameters(ctx, crop):
    """every group of tests/region_mask_cases.py: the triangles (both orientations, all equal, collinear, pixel centres and rows, far
    outside, +-10^6), the 27-vertex outline with its 12-vertex hole, two polygons and the bow-tie, holes inside / across / outside, the
    hulls of 22 points down to two and one, hull and plain polygons mixed; 16 x 16 and 37 x 29 under all twelve (grow, feather)"""
    w, h = crop
    every = crop in ((16, 16), (37, 29))
    lit, k = 0, 0
    for name, sizes, nh, bits_, rows in C.groups(w, h):
        params = C.PARAMS if every else [C.PARAMS[(k + 5 * j) % 12] for j in range(2)]
        k += 1
        for grow, feather in params:
            got, host, flags = draw_at(ctx, rows, sizes, nh, bits_, w, h, grow, feather)
            maps, wflags = C.expected_maps(w, h, name, grow, feather)
            assert np.array_equal(flags, wflags), (name, grow, feather)
            assert np.array_equal(got, with_maps(host, maps)), (name, grow, feather, np.argwhere(got != with_maps(host, maps))[:5])
            lit += int((maps > 0).sum())
    assert lit > 0


@pytest.mark.parametrize("n", [1, 3, 65])
def test_row_counts(ctx, n):
    """N = 1, 3 and 65 rows of the outline with its hole, each under a similarity of its own: 112 x 112 and 67 x 63 (16 bytes per lane;
    4221 bytes per map, so every map but the first begins inside a piece), 5 x 7 and 131 x 3 (4 bytes per lane)"""
    for (w, h), (grow, feather) in zip([(112, 112), (67, 63), (5, 7), (131, 3)], [(2.5, 4.0), (0.0, 0.0), (2.5, 0.5), (0.0, 16.0)]):
        name, sizes, nh, bits_ = OUTLINE
        base = next(g for g in C.groups(w, h) if g[0] == name)[4][3][1]                     # the outline in crop space (identity M)
        rows = [(C.sim(w, h, 100 + r), None) for r in range(n)]
        rows = [(M, C.to_frame(M, base + [r % 5 - 2, r % 3 - 1])) for r, (M, _) in enumerate(rows)]
        got, host, flags = draw_at(ctx, rows, sizes, nh, bits_, w, h, grow, feather)
        maps, wflags = R.masks(np.stack([M for M, _ in rows]), np.stack([p for _, p in rows]), sizes, nh, bits_, w, h, grow, feather)
        assert np.array_equal(flags, wflags) and not flags.any()
        assert np.array_equal(got, with_maps(host, maps)), (w, h, n)
        assert all(m.any() for m in maps) and (min(w, h) < 63 or ((maps == 255).any() and (maps == 0).any()))


def test_flagged_rows_leave_their_neighbours_alone(ctx):
    """a vertex beyond 2^20, a NaN, an infinity: zeros and SDM_REGION_NONFINITE; d == 0 and a NaN in M: zeros and SDM_ALIGN_DEGENERATE;
    the rows between them are drawn as if alone"""
    w, h = 37, 29
    good = next(g for g in C.groups(w, h) if g[0] == "triangle")[4][:6]
    rows = []
    for k, (M, p, _) in enumerate(FLAGGED):
        rows += [good[k], (M, p)]
    rows.append(good[5])
    got, host, flags = draw_at(ctx, rows, [3], 0, 0, w, h, 2.5, 4.0)
    maps, wflags = R.masks(np.stack([M for M, _ in rows]), np.stack([p for _, p in rows]), [3], 0, 0, w, h, 2.5, 4.0)
    assert flags.tolist() == wflags.tolist() and flags[1::2].tolist() == [f for _, _, f in FLAGGED] and not flags[0::2].any()
    assert np.array_equal(got, with_maps(host, maps))
    assert not maps[1::2].any() and all(m.any() for m in maps[0:9:2])


def landmark_rows_all(sims, w, h, seed):
    """N x 2L rows: the LM landmarks on the template, the others spread over the crop, all seen through each row's similarity"""
    rng = np.random.default_rng(seed)
    crop = np.stack([rng.uniform(0, w, L), rng.uniform(0, h, L)], 1)
    crop[LM] = template(w, h)
    return K.landmark_rows(sims, crop, np.arange(L), L)


def points_of(x, verts):
    v = np.asarray(verts)
    return np.ascontiguousarray(np.stack([x[:, v], x[:, L + v]], -1))


def test_fit_form_on_ragged_frames(ctx):
    """the current rows on ragged frames of all formats: the matrices and flags are align_crops_tensor's, the bytes the restatement's on
    those matrices; a NaN landmark among the vertices, a degenerate fit; _at with the returned matrices and the rows' points gives the
    same bytes"""
    buf, frames = K.place(K.RAGGED, 5)
    idx = [0, 1, 4, 0, 1, 4, 1]
    w, h = 37, 29
    kept = install(ctx, buf, frames, idx, w, h, 21)
    sims = K.similarities(frames, idx, w, h, 21)
    x = landmark_rows_all(sims, w, h, 22)
    polys, holes, hull = [[0, 1, 2, 4, 5, 7, 8], [10, 11, 13, 14]], [[16, 17, 18, 19, 20]], [0, 2]
    verts = [v for p in polys + holes for v in p]
    assert not set(verts) & set(LM.tolist())
    x[2, verts[3]] = np.nan                                                  # row 2: a vertex landmark that the fit does not use
    x[5, LM] = 7.0                                                           # row 5: the fitted landmarks coincide
    x[5, L + LM] = 9.0
    ctx.set_x(x)
    t = template(w, h)
    _, m0, f0 = ctx.align_crops_tensor(LM, t, w, h, dtype="uint8", layout="nhwc", channels=1)
    for grow, feather in ((0.0, 0.0), (2.5, 16.0)):
        dev, host, view = guarded_out(len(idx), w, h, 9)
        out, mats, flags = ctx.align_region_mask(LM, t, w, h, polys, holes, hull, grow, feather, out=view)
        assert np.array_equal(bits(mats), bits(m0))
        want_flags = f0.copy()
        want_flags[2] |= R.NONFINITE
        assert np.array_equal(flags, want_flags) and flags[5] == A.DEGENERATE and (f0 & A.PARTIAL).any()
        sizes, bits_ = [len(p) for p in polys + holes], sum(1 << g for g in hull)
        maps, rflags = R.masks(m0, points_of(x, verts), sizes, len(holes), bits_, w, h, grow, feather, flags_in=f0)
        assert np.array_equal(rflags, want_flags)
        got = dev.cpu().numpy()
        assert np.array_equal(got, with_maps(host, maps))
        assert not maps[2].any() and not maps[5].any() and all(maps[r].any() for r in (0, 1, 3, 4, 6))
        # the explicit form: no PARTIAL is evaluated, the bytes are the same
        dev2, host2, view2 = guarded_out(len(idx), w, h, 9)
        _, f_at = ctx.align_region_mask_at(mats, points_of(x, verts), w, h, sizes, len(holes), hull, grow, feather, out=view2)
        assert np.array_equal(f_at, want_flags & ~A.PARTIAL) and np.array_equal(dev2.cpu().numpy(), got)
    assert np.array_equal(kept[0].cpu().numpy(), buf)                        # the frames are only read
    assert np.array_equal(bits(ctx.get_x()), bits(x))                        # and so are the rows
    ctx.align_set_source_frames(None)
    ctx.set_sample_image_index(None)


def random_model(seed=77):
    rng = np.random.default_rng(seed)
    regs = [LinearRegressor() for _ in PARAMS]
    for reg, p in zip(regs, PARAMS):
        reg.x = rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(f32)
    return detection_model(SupervisedDescentOptimiser(regs), MEAN, IDS, PARAMS, ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS), rng


def test_through_the_paste(built):
    """a tracker step on three small colour frames, the crops, the region masks of the same rows, the paste with them as its opacity:
    the frames equal tests/paste_ref.py given the restatement's masks, on every byte"""
    import torch
    model, rng = random_model()
    colour = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (29, 37, 3), dtype=np.uint8),
              rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)]
    dev = [torch.from_numpy(c).cuda() for c in colour]
    tr = model.tracker(3)
    ids = np.arange(3)
    tr.start(ids, np.array([[20, 8, 30, 30], [6, 3, 24, 24], [14, 6, 28, 28]]))
    tr.step(ids, dev)
    x, m0, f0 = model.aligned_crops_tensor(16, frames=dev, dtype="uint8")
    regions, holes = ["face"], ["mouth_outer", "right_eye"]
    masks, mm, mf = model.region_masks(16, regions, holes, grow=1.0, feather=3.0)
    assert np.array_equal(bits(mm), bits(m0)) and np.array_equal(mf, f0) and not (mf & (A.DEGENERATE | R.NONFINITE)).any()
    pts = model.region_points(regions, holes)
    assert pts.shape == (3, 22 + 4 + 6, 2)
    want_masks, _ = R.masks(m0, pts, [22, 4, 6], 2, 1, 16, 16, 1.0, 3.0, flags_in=f0)
    assert np.array_equal(masks.cpu().numpy(), want_masks)
    assert (want_masks == 255).any() and all((m == 0).any() and ((m > 0) & (m < 255)).any() for m in want_masks)
    # rows that are no longer current: the matrices and the points of that moment
    later, _, _ = model.region_masks(16, regions, holes, grow=1.0, feather=3.0, matrices=m0, points=pts)
    assert np.array_equal(later.cpu().numpy(), want_masks)
    y = (255 - x).contiguous()                                               # the "network"
    dst = [torch.from_numpy(c).cuda() for c in colour]
    mats, flags = model.paste_crops_tensor(y, frames=dst, mask=masks)
    assert np.array_equal(bits(mats), bits(m0))
    for s in range(3):
        want = colour[s].copy()
        P.paste_row(want, T.BGR, m0[s], y[s].cpu().numpy(), want_masks[s])
        plain = colour[s].copy()
        P.paste_row(plain, T.BGR, m0[s], y[s].cpu().numpy(), None)
        assert (want != colour[s]).any() and (want != plain).any()
        assert np.array_equal(dst[s].cpu().numpy(), want), s
    model.optimised_model.ctx.close()


def test_refusals(built):
    """every refusal of the contract: SDM_ERR_INVALID, the output buffer keeps its noise, the current rows stay, and a detect and a valid
    call behind them give what they gave before"""
    import torch
    model, rng = random_model(78)
    c = model.optimised_model.ctx
    gray = [torch.from_numpy(rng.integers(0, 256, (48, 64), dtype=np.uint8)).cuda(),
            torch.from_numpy(rng.integers(0, 256, (29, 37), dtype=np.uint8)).cuda()]
    boxes = np.array([[20, 8, 30, 30], [6, 3, 24, 24]])
    rows0 = model.detect_batch(gray, boxes)
    w, h = 16, 16
    t = template(w, h)
    polys, holes = [[0, 1, 2, 4], [5, 7, 8]], [[10, 11, 13]]
    dev, host, view = guarded_out(2, w, h, 11)
    good, mats, flags = c.align_region_mask(LM, t, w, h, polys, holes, [1], 1.0, 2.0, out=view)
    good_bytes = dev.cpu().numpy()
    assert (good_bytes != host).any()

    dev, host, view = guarded_out(2, w, h, 11)
    lib, hnd = c._lib, c._h
    lm32, t32 = np.ascontiguousarray(LM, np.int32), np.ascontiguousarray(t)
    v32 = np.array([v for p in polys + holes for v in p], np.int32)
    m32 = np.ascontiguousarray(mats.reshape(-1, 6))
    p32 = np.ascontiguousarray(np.stack([rows0[:, v32], rows0[:, L + v32]], -1).astype(f32))

    def reg(sizes=(4, 3, 3), n_pol=None, nh=1, hb=2, grow=1.0, feather=2.0, null_sizes=False):
        arr = (ctypes.c_int * len(sizes))(*sizes)
        r = _lib.SdmRegionMask(None if null_sizes else arr, len(sizes) if n_pol is None else n_pol, nh, hb, grow, feather)
        r._keep = arr
        return r

    def fit(lm=lm32, tm=t32, k=LM.size, cw=w, chh=h, v=v32, r=reg(), o=view.data_ptr()):
        rc = lib.sdm_align_region_mask(hnd, None if lm is None else lm.ctypes.data, None if tm is None else tm.ctypes.data, k, cw, chh,
                                       None if v is None else v.ctypes.data, None if r is None else ctypes.byref(r), ctypes.c_void_p(o), None, None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    def at(m=m32, p=p32, n_rows=2, cw=w, chh=h, r=reg(), o=view.data_ptr()):
        rc = lib.sdm_align_region_mask_at(hnd, None if m is None else m.ctypes.data, None if p is None else p.ctypes.data, n_rows, cw, chh,
                                          None if r is None else ctypes.byref(r), ctypes.c_void_p(o), None)
        if rc:
            raise SdmError(rc, lib.sdm_last_error().decode())

    both = []
    for call in (fit, at):
        both += [
            lambda call=call: call(r=None), lambda call=call: call(r=reg(null_sizes=True)),
            lambda call=call: call(r=reg(n_pol=0)), lambda call=call: call(r=reg(n_pol=-1)), lambda call=call: call(r=reg(sizes=(3,) * 9, nh=0, hb=0)),
            lambda call=call: call(r=reg(sizes=(2, 4, 4))), lambda call=call: call(r=reg(sizes=(129, 3, 3))),
            lambda call=call: call(r=reg(sizes=(128, 128, 3), nh=0, hb=0)),                                   # P = 259
            lambda call=call: call(r=reg(nh=-1)), lambda call=call: call(r=reg(nh=3)),
            lambda call=call: call(r=reg(hb=8)), lambda call=call: call(r=reg(hb=1 << 31)),
            lambda call=call: call(r=reg(grow=np.nan)), lambda call=call: call(r=reg(grow=np.inf)), lambda call=call: call(r=reg(grow=1024.5)),
            lambda call=call: call(r=reg(grow=-1025.0)), lambda call=call: call(r=reg(feather=np.nan)), lambda call=call: call(r=reg(feather=-0.5)),
            lambda call=call: call(r=reg(feather=1025.0)), lambda call=call: call(r=reg(feather=np.inf)),
            lambda call=call: call(o=0), lambda call=call: call(o=view.data_ptr() + 8),                      # out_dev NULL, misaligned
            lambda call=call: call(cw=0), lambda call=call: call(chh=1025),
        ]
    cases = both + [
        # the fit form: what sdm_align_crops_tensor refuses of the landmarks, the template and K; the vertex indices
        lambda: fit(k=1), lambda: fit(k=L + 1), lambda: fit(lm=None), lambda: fit(tm=None), lambda: fit(lm=np.array([3, 3, 9, 12, 15], np.int32)),
        lambda: fit(lm=np.array([3, L, 9, 12, 15], np.int32)), lambda: fit(tm=np.full_like(t32, 2.0)),
        lambda: fit(tm=np.where(np.arange(5)[:, None] == 1, np.nan, t32).astype(f32)),
        lambda: fit(v=None), lambda: fit(v=np.where(np.arange(10) == 4, L, v32).astype(np.int32)),
        lambda: fit(v=np.where(np.arange(10) == 9, -1, v32).astype(np.int32)),
        # the _at form
        lambda: at(m=None), lambda: at(p=None), lambda: at(n_rows=0), lambda: at(n_rows=-2),
    ]
    for f in cases:
        assert code(f) == -1
    assert np.array_equal(dev.cpu().numpy(), host)                                  # nothing was launched
    assert np.array_equal(bits(c.get_x()), bits(rows0))                             # the current rows stay
    fresh = Context(0)
    try:
        assert code(fresh.align_region_mask, LM, t, w, h, polys, holes, [1], 1.0, 2.0) == -1      # no geometry, no rows
        out, fl = fresh.align_region_mask_at(mats, p32, w, h, [4, 3, 3], 1, [1], 1.0, 2.0)        # the _at form needs neither
        assert np.array_equal(out.cpu().numpy().reshape(-1), good_bytes[64:-64]) and np.array_equal(fl, flags & ~A.PARTIAL)
    finally:
        fresh.close()
    # a valid call and a detect behind the refusals give what they gave before them
    out2, m2, f2 = c.align_region_mask(LM, t, w, h, polys, holes, [1], 1.0, 2.0, out=view)
    assert np.array_equal(dev.cpu().numpy(), good_bytes) and np.array_equal(bits(m2), bits(mats)) and np.array_equal(f2, flags)
    assert np.array_equal(bits(model.detect_batch(gray, boxes)), bits(rows0))
    c.close()


def test_python_layer_argument_errors(ctx):
    import torch
    t = template(16, 16)
    ctx.set_x(np.zeros((2, 2 * L), f32))
    with pytest.raises(ValueError):
        ctx.align_region_mask(LM, t[:4], 16, 16, [[0, 1, 2]])
    with pytest.raises(ValueError):
        ctx.align_region_mask(LM, t, 16, 16, [[0, 1, 2]], out=torch.zeros((2, 16, 15), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ctx.align_region_mask(LM, t, 16, 16, [[0, 1, 2]], hull=[1])
    with pytest.raises(ValueError):
        ctx.align_region_mask_at(np.zeros((2, 2, 3), f32), np.zeros((2, 4, 2), f32), 16, 16, [3])
