"""Frame geometry beyond 256 x 256 for the kernels that came after tests/test_gpu_frame_geometry.py (tests/frame_geometry_cases.py,
"the paste cases"): the four pastes, which WRITE into the caller's frames in place -- rigid, filtered, NV12 (luma and 4:2:0 chroma) and
piecewise-affine -- on the frames of that module (pitches that carry a byte offset past 2^16, 2^24 and over INT_MAX, 65 535 and 65 600
rows, 70 000 columns, frames more than 2^32 bytes apart, NV12 surfaces with a far chroma plane, of odd size and with a chroma plane
BEFORE the luma), and the three readers: the area-filtered crop, the warped crop and the upright chip.  Every frame is a view into the
ONE device buffer of 255s; everything is compared bit for bit with the numpy restatements (paste_ref, paste_area_ref, paste_nv12_ref,
warp_paste_ref on a window around every row; align_area_ref, warp_ref, upright_ref), there is no tolerance anywhere.

How a paste case is checked: every view is read back and compared with the restatement's bytes; the views are set to 255 again; then
the WHOLE buffer must be 255 -- a store anywhere in 4.5 GiB shows, because no tensor element decodes above 200 and no opacity-map
entry lies between 1 and 63, so that a stray blend over 255 gives at most 241.  What keeps a case from passing by accident
(frame_geometry_cases.paste_unmet) is asserted without a GPU in test_case_table."""
import contextlib

import numpy as np
import pytest

import align_area_ref as AR
import align_ref as A
import align_tensor_ref as T
import frame_geometry_cases as G
import paste_cases as PC
import paste_ref as P
import upright_ref as U
import warp_paste_ref as WP
import warp_ref as WR
from test_gpu_frame_geometry import CROP, FMT, LMS, big, bind, bits, disjoint, model, nv12_pixels, placed, views_of  # noqa: F401
from superviseddescent_amd import alignment_template

gpu = pytest.mark.gpu
f32 = np.float32
MEAN, L = G.MEAN, G.L
CHUNK = 2 ** 28
FILTER_ARGS = dict(filter="area", max_samples=16, min_scale=1.0)


# ---- no GPU: the windowed restatements, the table ---------------------------------------------------------------------------------------
SMALL = {"rigid": [(37, 29, "bgr"), (64, 48, "rgba"), (33, 21, "gray")],                 # (the frames of tests/paste_cases.py,
         "area": [(37, 29, "bgr"), (64, 48, "rgba"), (33, 21, "gray")],                  #  tests/paste_nv12_cases.py and
         "nv12": [(37, 29, "nv12"), (64, 48, "nv12"), (33, 21, "nv12")],                 #  tests/warp_cases.py that hold a window
         "nv12 area": [(37, 29, "nv12"), (64, 48, "nv12"), (33, 21, "nv12")],            #  with a margin of 16 pixels)
         "warp": [(40, 36, "gray"), (37, 33, "bgr"), (48, 40, "rgba")]}


@pytest.mark.parametrize("family", G.FAMILIES)
def test_windowed_reference_equals_whole_frame_reference(family):
    """the restatement on a window with a non-zero origin gives the bytes of the whole-frame restatement there, and the whole-frame
    restatement leaves the rest of the frame as it was: small frames of the existing tests, small crops, S = 1 and 3"""
    frames = [G.frame(w, h, w * G.BPP[fmt] + 3, 0, fmt) for w, h, fmt in SMALL[family]]
    idx = [0, 1, 2, 1, 0, 1]                                                   # (the 37- and 33-pixel frames lie wholly inside their windows)
    places = [(0.62 * frames[i]["w"], 0.6 * frames[i]["h"]) for i in idx[:3]] + [(42, 28), (34, 26), (3, 2)]
    scales = [2.6, 1.0, 2.6, 2.6, 1.7, 1.0] if family.endswith("area") else [2.4, 1.0, 2.2, 2.0, 2.4, 1.0]
    for k in range(3):                                                         # (no map, one for all rows, one per row)
        c = G.paste_case(k, "0", family, frames, idx, places, 16, 16, "", None, scales=scales)
        pixels = G.paste_pixels(c)
        whole, _ = G.paste_reference(c, pixels, whole=True)
        win, info = G.paste_reference(c, pixels)
        inside = [tuple(np.zeros(q.shape[:2], bool) for q in p) if isinstance(p, tuple) else np.zeros(p.shape[:2], bool) for p in pixels]
        shifted = outside = 0
        for r, rec in enumerate(info):
            (x0, y0), (h, w) = rec["origin"], rec["touched"].shape
            shifted += x0 > 0 and y0 > 0 and bool(rec["changed"].any())
            m = inside[idx[r]]
            if isinstance(m, tuple):
                m[0][y0:y0 + h, x0:x0 + w] = True
                m[1][y0 // 2:(y0 + h + 1) // 2, x0 // 2:(x0 + w + 1) // 2] = True
            else:
                m[y0:y0 + h, x0:x0 + w] = True
        assert shifted >= 2 and (family.endswith("area")) == (max(rec["S"] for rec in info) == 3)
        flat = lambda v: [a for p in v for a in (p if isinstance(p, tuple) else (p,))]
        for a, b, before, m in zip(flat(whole), flat(win), flat(pixels), flat(inside)):
            assert np.array_equal(a[m], b[m]) and (a[m] != before[m]).any()   # the window: the whole-frame result's bytes
            assert np.array_equal(a[~m], before[~m]) and np.array_equal(b[~m], before[~m])                     # the rest: unchanged
            outside += int((~m).sum())
        assert outside > 300


def placement_frames(c):
    return G.paste_placement(c, G.paste_pixels(c))[0]


def test_case_table():
    for case, what, value, lo, hi in G.table():
        assert lo < value <= hi, (case, what, value, lo, hi)
    cases = G.paste_cases()
    used = set()
    for name, c in cases.items():
        frames = placement_frames(c)
        for f in frames:
            assert f["off"] >= 4096 and f["off"] + G.extent(f) + 4096 <= G.BUF_BYTES and f["pitch"] >= f["w"] * G.BPP[f["fmt"]], (name, f)
        assert disjoint(frames), name
        assert len(c["idx"]) <= 12 and c["family"] in G.FAMILIES
        # no element decodes above 200; an opacity is 0 or at least 64
        assert P.decode(P.as_hwc(c["x"][0], c["layout"], c["channels"]), PC.SCALES, PC.BIASES).max() <= 200
        assert all(P.decode(P.as_hwc(x, c["layout"], c["channels"]), PC.SCALES, PC.BIASES).max() <= 200 for x in c["x"])
        assert c["alpha"] is None or ((c["alpha"] == 0) | (c["alpha"] >= 64)).all()
        assert G.paste_unmet(name) == [], (name, G.paste_unmet(name))
        assert not (G.paste_flags(c) & A.DEGENERATE).any()
        used.add((c["dtype"], c["layout"], c["order"], c["channels"], "null" if c["alpha"] is None else "shared" if c["alpha"].ndim == 2 else "rows"))
    for i, values in enumerate((("uint8", "float16", "float32"), ("nhwc", "nchw"), ("bgr", "rgb"), (1, 3), ("null", "shared", "rows"))):
        assert {u[i] for u in used} == set(values)
    for fam in G.FAMILIES:                                                     # every family on the frame whose h * pitch is over INT_MAX
        assert "2 over INT_MAX, " + fam in cases
    # the filtered rows: S = 1, 2, 3 and the cap; the capped row's crop outsizes its face 20 times
    S = {rec["S"] for name in cases if name.endswith("area") for rec in G.paste_expected(name)[2]}
    assert S >= {1, 2, 3, 16}
    # a case that lacks a condition is caught: without its rows beyond column 65 536 the wide frame has no changed byte there
    assert G.paste_unmet("4 width 70000, rigid", rows=[0, 4]) == ["a row across the right border", "a row across the top border",
                                                                   "a changed byte beyond the boundary"]
    assert "a filtered row with mu >= 2^20" in G.paste_unmet("4 width 70000, area", rows=[0, 2, 3, 4, 5, 6])


# ---- the device ------------------------------------------------------------------------------------------------------------------------
def stray(big):
    """[(first byte, bytes)] per 2^28 chunk of the buffer that is not all 255, reduced on the device; such a chunk is set to 255 again"""
    bad = []
    for at in range(0, G.BUF_BYTES, CHUNK):
        part = big[at:at + CHUNK]
        if int(part.min()) != 255:
            where = (part != 255).nonzero()
            bad.append((at + int(where[0]), int(where.numel())))
            part.fill_(255)
    return bad


@contextlib.contextmanager
def checked(big, frames, pixels):
    """test_gpu_frame_geometry.placed, and behind it -- the views are 255 again -- the WHOLE buffer must be 255.  A case that fails
    inside still has its stray bytes repaired, so that the next case starts from a clean buffer and fails or passes on its own."""
    try:
        with placed(big, frames, pixels) as lst:
            yield lst
    except BaseException:
        stray(big)
        raise
    bad = stray(big)
    assert not bad, "stores outside the frames: (first byte, bytes) per 2^28 chunk %s" % bad


def device_lists(big, c):
    base = big.data_ptr()
    lst = [(base + f["off"], f["w"], f["h"], f["pitch"], f["fmt"]) for f in c["frames"]]
    chroma = [base + f["uv_off"] if "uv_off" in f else None for f in c["frames"]]
    return lst, (chroma if any("uv_off" in f for f in c["frames"]) else None)


def read_back(big, c, want, what):
    frames, wpix = G.paste_placement(c, want)
    for i, (f, w) in enumerate(zip(frames, wpix)):
        for plane, (v, a) in enumerate(zip(views_of(big, f), w if isinstance(w, tuple) else (w,))):
            got = v.cpu().numpy()
            assert np.array_equal(got, a), (what, "frame %d plane %d" % (i, plane), "%d bytes differ" % int((got != a).sum()))


def call_at(ctx, big, c):
    """the _at form of the case's family; returns (flags, S or None)"""
    import torch
    lst, chroma = device_lists(big, c)
    y = torch.from_numpy(c["x"]).cuda()
    mask = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
    spec = G.paste_spec(c)
    if c["family"] == "warp":
        idx, t, tri, lab = G.mesh(c["cw"], c["ch"])
        ctx.warp_set_mesh(idx, t, tri, c["cw"], c["ch"])
        assert np.array_equal(ctx.warp_labels(), lab)
        return ctx.warp_paste_tensor_at(G.paste_points(c), y, lst, image_index=c["idx"], mask=mask, **spec), None
    kw = dict(spec, **(FILTER_ARGS if c["filter"] is not None else {}))
    if chroma is not None:
        kw["chroma"] = chroma
    res = ctx.align_paste_tensor_at(c["mats"], y, lst, image_index=c["idx"], mask=mask, **kw)
    return res if c["filter"] is not None else (res, None)


@gpu
@pytest.mark.parametrize("name", list(G.paste_cases()))
def test_paste_at(model, big, name):
    c = G.paste_cases()[name]
    pixels, want, info = G.paste_expected(name)
    ctx = bind(model)
    frames, ppix = G.paste_placement(c, pixels)
    with checked(big, frames, ppix):
        flags, S = call_at(ctx, big, c)
        ctx.synchronize()
        assert np.array_equal(flags, G.paste_flags(c)), name
        assert S is None or S.tolist() == [rec["S"] for rec in info], name
        read_back(big, c, want, name)
        if "twins" in name:                                                    # a surface and its twin: the same luma and chroma bytes
            v = [[p.cpu().numpy() for p in views_of(big, f)] for f in c["frames"]]
            for a, b in ((0, 1), (2, 3)):
                assert np.array_equal(v[a][0], v[b][0]) and np.array_equal(v[a][1], v[b][1]) and (v[a][1] != pixels[a][1]).any()


# one fit-form call per family behind detect_batch, on the frames more than 2^32 bytes apart and on the frame over INT_MAX
@gpu
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("where", ["5 far apart", "2 over INT_MAX"])
def test_paste_fit_form_behind_detect_batch(model, big, family, where):
    import torch
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()[where]
    nv12 = family.startswith("nv12")
    frames = [dict(f, fmt="nv12" if nv12 else "gray") for f in frames]
    pixels = [(im, nv12_pixels(k)[1]) if nv12 else im for k, im in enumerate(images)]
    cw = ch = 64 if family.endswith("area") else CROP
    k = 40 + G.FAMILIES.index(family)
    c = G.paste_case(k, where[0], family, frames, idx, [(0, 0)] * len(idx), cw, ch, borders, None)
    ctx = bind(model)
    with checked(big, frames, pixels) as lst:
        ctx.set_frames_device(lst)
        ctx.set_sample_image_index(idx)
        ctx.set_x(G.level0(where)[0])
        final = ctx.detect_batch()
        y = torch.from_numpy(c["x"]).cuda()
        mask = None if c["alpha"] is None else torch.from_numpy(c["alpha"]).cuda()
        spec = G.paste_spec(c)
        if family == "warp":
            midx, t, tri, lab = G.mesh(cw, ch)
            ctx.warp_set_mesh(midx, t, tri, cw, ch)
            mats, flags = ctx.warp_paste_tensor(y, lst, mask=mask, **spec)
            c["points"] = WP.points_of(final, midx)
            assert np.array_equal(bits(mats.reshape(len(idx), -1, 6)), bits(WP.matrices(c["points"], t, tri)))
        else:
            tmpl = alignment_template(MEAN, LMS, cw, ch, 0.2)
            res = ctx.align_paste_tensor(LMS, tmpl, y, lst, mask=mask, **dict(spec, **(FILTER_ARGS if c["filter"] else {})))
            c["mats"], flags = res[0], res[1]
            _, m0, f0 = ctx.align_crops_tensor(LMS, tmpl, cw, ch, dtype="uint8", layout="nhwc", channels=1)      # the crop call's fit
            assert np.array_equal(bits(c["mats"]), bits(m0)) and np.array_equal(flags, f0)
        ctx.synchronize()
        want, info = G.paste_reference(c, pixels)
        assert np.array_equal(flags, G.paste_flags(c))
        if c["filter"]:
            assert res[2].tolist() == [rec["S"] for rec in info] and res[2].max() > 1      # (a crop of 64 on faces of 60 to 72 pixels)
        assert sum(int(rec["changed"].sum()) for rec in info) > 2000
        read_back(big, c, want, (where, family))
        ctx.upload_images([np.zeros((4, 4), np.uint8)])


# ---- the readers that came after the first geometry module: the area-filtered crop, the warped crop, the upright chip -------------------------
READER_SPECS = [dict(dtype="float16", layout="nchw", channels=3, order="rgb", scale=PC.SCALES, bias=PC.BIASES),
                dict(dtype="uint8", layout="nhwc", channels=1)]
READER_SETS = (["1 " + n for n in G.CASE1] + ["1 largest fused stride", "3 height 65535", "3 height 65600", "4 width 70000", "5 far apart"])


def check_new_crops(ctx, lst, host, idx):
    """the sibling of test_gpu_frame_geometry.check_crops for the two crop calls that came later, on the current rows: the area-filtered
    crop against align_area_ref, the warped crop on the RCR-22 mesh against warp_ref, through the device's own matrices"""
    tmpl = alignment_template(MEAN, LMS, CROP, CROP, 0.2)
    ctx.align_set_source_frames(lst)
    midx, t, tri, lab = G.mesh(CROP, CROP)
    ctx.warp_set_mesh(midx, t, tri, CROP, CROP)
    assert np.array_equal(ctx.warp_labels(), lab)
    for spec in READER_SPECS:
        _, m0, f0 = ctx.align_crops_tensor(LMS, tmpl, CROP, CROP, **spec)
        got, mats, flags, S = ctx.align_crops_tensor(LMS, tmpl, CROP, CROP, filter="area", **spec)
        assert np.array_equal(bits(mats), bits(m0)) and np.array_equal(flags, f0) and not (flags & A.DEGENERATE).any()
        assert S.tolist() == [AR.samples(m) for m in mats] and S.max() > 1      # (faces of 60 to 72 pixels on a crop of 24: S = 3)
        got = got.cpu().numpy()
        for r, im in enumerate(idx):
            assert np.array_equal(bits(got[r]), bits(AR.tensor(host[im], mats[r], CROP, CROP, int(S[r]), **spec))), ("area", r, spec["dtype"])
        got, wm, wf = ctx.warp_crops_tensor(**spec)
        got = got.cpu().numpy()
        assert got.any() and not (wf & WR.DEGENERATE).any()
        for r, im in enumerate(idx):
            assert np.array_equal(bits(got[r]), bits(WR.tensor(host[im], wm[r].reshape(-1, 6), lab, **spec))), ("warp", r, spec["dtype"])
    ctx.align_set_source_frames(None)


@gpu
@pytest.mark.parametrize("name,fmt", [(n, "gray") for n in READER_SETS] + [("1 " + n, "nv12") for n in G.CASE1])
def test_filtered_and_warped_crops(model, big, name, fmt):
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()[name]
    ctx = bind(model)
    frames = [dict(f, fmt=fmt) for f in frames]
    pixels = [(im, nv12_pixels(k)[1]) if fmt == "nv12" else im for k, im in enumerate(images)]
    host = [T.Frame(FMT[fmt], *(p if isinstance(p, tuple) else (p,))) for p in pixels]
    with checked(big, frames, pixels) as lst:
        ctx.set_frames_device(lst)
        ctx.set_sample_image_index(idx)
        ctx.set_x(G.level0(name)[0])
        ctx.detect_batch()
        check_new_crops(ctx, lst, host, idx)
        for f, p in zip(frames, pixels):                                       # the source is only read
            assert all(np.array_equal(v.cpu().numpy(), a) for v, a in zip(views_of(big, f), p if isinstance(p, tuple) else (p,)))
        ctx.upload_images([np.zeros((4, 4), np.uint8)])


@gpu
def test_filtered_and_warped_crops_nv12_far_planes(model, big):
    """case 7's surfaces: the far chroma plane and the plane over INT_MAX beside their twins"""
    from test_gpu_frame_geometry import CASE7_FRAMES, CASE7_IDX, case7_boxes
    ctx = bind(model)
    pixels = [nv12_pixels(0), nv12_pixels(0), nv12_pixels(1), nv12_pixels(1)]
    host = [T.Frame(T.NV12, *p) for p in pixels]
    with checked(big, CASE7_FRAMES, pixels) as lst:
        ctx.set_frames_device(lst)
        ctx.set_sample_image_index(CASE7_IDX)
        ctx.set_x(G.aligned(case7_boxes()))
        ctx.detect_batch()
        check_new_crops(ctx, lst, host, CASE7_IDX)
        ctx.upload_images([np.zeros((4, 4), np.uint8)])


UPRIGHT_SETS = ["3 height 65600", "4 width 70000", "5 far apart", "1 pitch 2^18"]
ROLLS = np.array([0, 90, 17.3, -33, 180, 45, -90, 135, -150], f32)
CHIP, GUARD = 64, 8


@gpu
@pytest.mark.parametrize("name", UPRIGHT_SETS)
def test_upright_chips(model, big, name):
    """detect_batch(roll=) on the far frames: every chip byte for byte the restated warp of the row's frame, and chips, matrices, flags and
    landmarks those of the same call on a host upload of the same pixels"""
    images, boxes, idx, frames, borders, beyond, far = G.detect_cases()[name]
    rolls = ROLLS[np.arange(len(boxes)) % len(ROLLS)]
    ctx = bind(model)
    runs = []
    with checked(big, frames, images) as lst:
        for src in (lst, list(images)):
            res = model.detect_batch(src, boxes, idx, roll=rolls, chip=CHIP, guard=GUARD)
            runs.append((res,) + tuple(ctx.upright_get(chips=True)))
        ctx.upload_images([np.zeros((4, 4), np.uint8)])
    (res, M, flags, chips), (hres, hM, hflags, hchips) = runs
    assert np.array_equal(bits(M), bits(U.detect_setup(boxes, rolls, CHIP)[0]))
    for r, im in enumerate(idx):
        ref = U.chips(images[im], M[r], CHIP)
        assert np.array_equal(chips[r], ref), (name, r, int((chips[r] != ref).sum()))
    assert chips.any() and (flags & U.PARTIAL).any()                       # (the tall frame is 64 pixels wide: every chip of 64 is PARTIAL there)
    assert np.array_equal(chips, hchips) and np.array_equal(bits(M), bits(hM)) and np.array_equal(flags, hflags)
    assert np.array_equal(bits(res), bits(hres))
