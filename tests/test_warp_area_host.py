"""sdm_warp_crops_tensor_filtered without a device (include/sdm.h, "Warped faces, filtered"): what the shared case set covers, the
(Sx, Sy) rule, the identity of (1, 1) with the unfiltered restatement, how close the filtered warp comes to the box integral of every
pixel's footprint, and the per-triangle / per-pixel code of csrc/sdm_warp_area_device.h compiled for the host
(tests/cpp/warp_area_host.cpp, address and undefined-behaviour sanitizers, planes of exactly the frames' bytes) against the numpy
restatement (tests/warp_area_ref.py), bit for bit, for both offset widths."""
import struct

import numpy as np

import align_ref as A
import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import warp_area_cases as C
import warp_area_ref as WA
import warp_ref as R
from superviseddescent_amd import _lib

f32 = np.float32
up = lambda v: np.nextafter(f32(v), f32(np.inf))


def case_rows(w, h, mesh):
    buf, frames = C.place()
    idx, t, tri = C.MESHES[mesh](w, h)
    x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
    return buf, frames, idx, t, tri, x


def test_case_set_covers_what_it_must(built):
    """the conditions the device tests rely on, computed with the restatements alone"""
    for (w, h) in C.CROPS:
        buf, frames, idx, t, tri, x = case_rows(w, h, "rcr22")
        mats = R.matrices(x, idx, t, tri)
        flags = R.flags(x, idx, t, tri, [(frames[i]["w"], frames[i]["h"]) for i in C.ROWS])
        S = np.stack([WA.samples(m) for m in mats])                         # N x T x 2
        pairs = {tuple(p) for p in S.reshape(-1, 2)}
        print("crop %d x %d: %d pairs %s" % (w, h, len(pairs), sorted(pairs)))
        assert len(pairs) >= 6                                              # (a)
        assert any(a != b for a, b in pairs)                                # (b)
        assert any(len({tuple(p) for p in row}) >= 2 for row in S)          # (c) lanes of one wave diverge
        assert any((row == 1).all() for row in S) and any((row > 1).any() for row in S)        # (d)
        assert (flags & R.PARTIAL).any()                                    # (e)
        assert not (flags & (R.FOLDED | R.DEGENERATE)).any()                # (f)


def test_sample_rule():
    def S(m, **kw):
        return tuple(WA.samples(np.array(m, f32), **kw)[0])

    # exactly 4.0 and the next float above it, per axis and independently
    assert S([2, 0, 5, 0, 2, 7]) == (2, 2)
    m = np.array([2, 0, 0, 7e-4, 2, 0], f32)                                # cx2 = 4 + 4.9e-7, rounded: the float above 4
    assert WA.squares(m)[0, 0] == up(4.0) and WA.squares(m)[0, 1] == 4 and S(m) == (3, 2)
    assert S([0, 2, 0, 2, 0, 0]) == (2, 2)                                  # (a quarter turn: the columns swap roles)
    assert S([3, 1, 0, 0, 1, 0]) == (3, 2)                                  # a shear: cx2 = 9, cy2 = 2
    assert S([1, 3, 0, 0.5, 0, 0]) == (2, 3)                                # cx2 = 1.25, cy2 = 9
    # each operation rounded
    m = np.array([1.7, 0.3, 0, -0.9, 2.2, 0], f32)
    cx2 = f32(f32(m[0] * m[0]) + f32(m[3] * m[3]))
    cy2 = f32(f32(m[1] * m[1]) + f32(m[4] * m[4]))
    assert np.array_equal(WA.squares(m)[0], [cx2, cy2]) and S(m) == (2, 3)
    # a non-finite entry touches only the axis it enters
    assert S([np.nan, 0, 0, 3, 3, 0]) == (1, 3) and S([3, np.inf, 0, 3, 0, 0]) == (5, 1) and S([np.nan] * 6) == (1, 1)
    assert S([2e19, 0, 0, 2e19, 3, 0]) == (1, 3)                            # (cx2 overflows to inf)
    # the gate and the cap
    assert S([1.9, 0, 0, 0, 2.5, 0], min_scale=2.0) == (1, 3) and S([2, 0, 0, 0, 2.5, 0], min_scale=2.0) == (2, 3)
    assert S([4.5, 0, 0, 0, 3.5, 0], max_samples=3) == (3, 3) and S([4.5, 0, 0, 0, 1.5, 0], max_samples=4) == (4, 2)
    assert S([40, 0, 0, 0, 1, 0]) == (16, 1) and S([4, 0, 0, 0, 4, 0], max_samples=1) == (1, 1)
    # mode BILINEAR and a DEGENERATE row
    assert S([5, 0, 0, 0, 5, 0], mode=WA.BILINEAR) == (1, 1) and S([5, 0, 0, 0, 5, 0], degenerate=True) == (1, 1)
    # a similarity: Sx = Sy = the rigid call's S
    import align_area_ref as AR
    for s, ang in ((2.6, 31.0), (0.9, 5.0), (4.0, 0.0), (7.3, -44.0)):
        M = A.similarity(s, ang, 5, 7).astype(f32)
        assert S(M.reshape(6)) == (AR.samples(M),) * 2                      # (cy2 adds the same two squares in the other order)
    assert "sdm_warp_crops_tensor_filtered" in _lib.EXPORTED


def test_all_ones_is_the_unfiltered_restatement(built):
    w, h = C.CROPS[0]
    buf, frames, idx, t, tri, x = case_rows(w, h, "rcr22")
    lab = R.labels(t, tri, w, h)
    mats = R.matrices(x, idx, t, tri)
    ones = np.ones((len(tri), 2), np.int32)
    for r, im in enumerate(C.ROWS):
        frame = K.host_frame(buf, frames[im])
        a, b = R.warped(frame, mats[r], lab), WA.warped(frame, mats[r], lab, ones)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        if a[0] == "nv12":
            assert np.array_equal(a[2], b[2])


def ideal_box(img, mats, lab, n=32):
    """float64 box integral of the bilinear surface over every labelled pixel's footprint -- the parallelogram its own triangle's matrix
    makes of the pixel's square --, n x n midpoints; (values height x width, footprint inside the image)"""
    h, w = lab.shape
    H, W = img.shape
    g = img.astype(np.float64)
    o = (np.arange(n) + 0.5) / n - 0.5
    val, inside = np.zeros((h, w)), np.zeros((h, w), bool)
    for t in np.unique(lab):
        if t == R.NONE:
            continue
        M = np.asarray(mats, np.float64).reshape(-1, 2, 3)[t]
        ii, jj = np.nonzero(lab == t)
        fj, fi = jj[:, None, None] + o[None, None, :], ii[:, None, None] + o[None, :, None]
        sx = M[0, 0] * fj + M[0, 1] * fi + M[0, 2]
        sy = M[1, 0] * fj + M[1, 1] * fi + M[1, 2]
        inside[ii, jj] = ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).all((1, 2))
        x0, y0 = np.clip(np.floor(sx).astype(int), 0, W - 2), np.clip(np.floor(sy).astype(int), 0, H - 2)
        ax, ay = np.clip(sx - x0, 0, 1), np.clip(sy - y0, 0, 1)
        v = (1 - ax) * (1 - ay) * g[y0, x0] + ax * (1 - ay) * g[y0, x0 + 1] + (1 - ax) * ay * g[y0 + 1, x0] + ax * ay * g[y0 + 1, x0 + 1]
        val[ii, jj] = v.mean((1, 2))
    return val, inside


def test_closer_to_the_ideal_than_bilinear(built):
    """On uniform noise one bilinear sample says little about the mean over a footprint several pixels wide, while the average of Sx Sy
    samples spread over the footprint approaches it.  Mean |error| in levels against the float64 box integral over the labelled pixels
    whose footprint lies inside the frame, measured with the restatements (random 96 x 96 frame, 24 x 20 crop, the template sheared and
    bent as the case set's row 0, then scaled):
        single  scale 2.5   (3, 3)            filtered 1.86   unfiltered 29.34   (179 pixels)
        single  scale 4.3   (5, 5)            filtered 0.86   unfiltered 40.01   (174 pixels)
        rcr22   scale 2.5   (3, 2), (3, 3)    filtered 1.94   unfiltered 29.55   (111 pixels)
        rcr22   scale 4.3   (5, 3), (5, 5)    filtered 0.85   unfiltered 40.83   (111 pixels)
    The assertion asks for half of the measured gap, as tests/test_align_area_host.py's precedent would: filtered < unfiltered - gap / 2
    with the gap of the table rounded down (GAPS)."""
    img = np.random.default_rng(5).integers(0, 256, (96, 96), dtype=np.uint8)
    frame = T.Frame(T.GRAY, img)
    w, h = C.CROPS[0]
    frames = [dict(w=96, h=96)]
    for mesh in ("single", "rcr22"):
        idx, t, tri = C.MESHES[mesh](w, h)
        lab = R.labels(t, tri, w, h)
        for scale in (2.5, 4.3):
            x = C.rows_for(frames, [0], idx, t, w, h, 31, scales=[scale * 4.6 / min(96 / w, 96 / h)])
            mats = R.matrices(x, idx, t, tri)[0]
            S = WA.samples(mats)
            assert (S >= 2).all() and not R.flags(x, idx, t, tri, [(96, 96)])[0] & R.FOLDED
            ideal, inside = ideal_box(img, mats, lab)
            assert inside.sum() >= 40
            _, area, _ = WA.warped(frame, mats, lab, S)
            _, plain, _ = R.warped(frame, mats, lab)
            e_area, e_plain = np.abs(area[..., 0] - ideal)[inside].mean(), np.abs(plain[..., 0] - ideal)[inside].mean()
            print("%-6s scale %.1f  S %s: mean |error| against the box integral, filtered %.2f, unfiltered %.2f (%d pixels)"
                  % (mesh, scale, sorted({tuple(p) for p in S}), e_area, e_plain, inside.sum()))
            gap = GAPS[(mesh, scale)]
            assert e_area < e_plain - gap / 2


GAPS = {("single", 2.5): 27.0, ("single", 4.3): 39.0, ("rcr22", 2.5): 27.0, ("rcr22", 4.3): 39.0}


def border_matrices(f, w, h, T_):
    """T_ matrices that send sub-samples across every border of frame f at several anisotropic scales, a position beyond 2^20 and a NaN"""
    out = []
    for k in range(T_):
        dx, dy = [(-3.4, 1.2), (f["w"] - 2.0 * w + 3.7, 0.4), (0.6, -2.3), (1.1, f["h"] - 2.0 * h + 2.8)][k % 4]
        sx, sy = [(1.0, 1.0), (2.3, 1.4), (0.53, 3.1), (3.7, 3.7), (1.0, 2.0)][k % 5]
        out.append([sx, 0.07 * (k % 5), dx, -0.05 * (k % 3), sy, dy])
    m = np.array(out, f32)
    if T_ > 6:
        m[5, 2] = 3e6
        m[6, 0] = np.nan
    return m


def test_host_build_of_the_warp_area_code_under_sanitizers(built, tmp_path):
    """the device functions, compiled for the host with their own main, on planes of exactly the frames' bytes; the program runs every
    segment through the 32-bit and the 64-bit offset path (WIDE false and true) and exits 1 when they differ"""
    exe = B.host_program("warp_area_host", tmp_path)
    scale, bias = np.array([1 / 58.395, 1 / 57.12, 1 / 57.375], f32), np.array([-2.1179, -2.0357, -1.8044], f32)
    # ---- the rule on hand-picked matrices
    rules = [([2, 0, 5, 0, 2, 7], 0, 1, 16, 1.0), ([2, 0, 0, 7e-4, 2, 0], 0, 1, 16, 1.0), ([3, 1, 0, 0, 1, 0], 0, 1, 16, 1.0),
             ([np.nan, 0, 0, 3, 3, 0], 0, 1, 16, 1.0), ([3, np.inf, 0, 3, 0, 0], 0, 1, 16, 1.0), ([2e19, 0, 0, 2e19, 3, 0], 0, 1, 16, 1.0),
             ([1.9, 0, 0, 0, 2.5, 0], 0, 1, 16, 2.0), ([2, 0, 0, 0, 2.5, 0], 0, 1, 16, 2.0), ([4.5, 0, 0, 0, 3.5, 0], 0, 1, 3, 1.0),
             ([40, 0, 0, 0, 1, 0], 0, 1, 16, 1.0), ([5, 0, 0, 0, 5, 0], 0, 0, 16, 1.0), ([5, 0, 0, 0, 5, 0], R.DEGENERATE, 1, 16, 1.0),
             ([5, 0, 0, 0, 5, 0], R.PARTIAL | R.FOLDED, 1, 16, 1.0), ([5, 0, 0, 0, 5, 0], 0, 1, 16, 1e30)]
    head = [struct.pack("<i", len(rules))] + [np.array(m, f32).tobytes() + struct.pack("<iiif", fl, mode, cap, gate) for m, fl, mode, cap, gate in rules]
    want_rules = np.concatenate([WA.samples(np.array(m, f32), bool(fl & R.DEGENERATE), mode, cap, gate) for m, fl, mode, cap, gate in rules])
    assert tuple(want_rules[1]) == (3, 2) and tuple(want_rules[8]) == (3, 3) and tuple(want_rules[12]) == (5, 5)
    # ---- the pixels: the case set through fitted matrices (three filters) and through matrices that cross every border
    cases, blob, seen, pairs = [], [b""], set(), set()

    def add(frame_bytes, f, host, mats, lab, w, h, filt):
        mode, cap, gate = filt
        b0, b1 = K.plane_bytes(f)
        p0, p1 = frame_bytes
        blob.append(struct.pack("<8i", f["fmt"], f["w"], f["h"], f["stride"], f["stride"] if b1 else 0, w, h, len(mats))
                    + np.asarray(mats, f32).tobytes() + lab.tobytes() + scale.tobytes() + bias.tobytes()
                    + struct.pack("<iiif", 0, mode, cap, gate) + struct.pack("<i", b0) + p0 + struct.pack("<i", b1) + p1)
        S = WA.samples(mats, False, mode, cap, gate)
        cases.append((host, np.asarray(mats, f32), lab, S))
        seen.add(f["fmt"])
        pairs.update((f["fmt"],) + tuple(p) for p in S[np.unique(lab[lab != R.NONE])])

    buf, frames = C.place()
    swapped = {T.BGR: T.RGB, T.RGBA: T.BGRA}
    for ci, (w, h) in enumerate(C.CROPS):
        idx, t, tri = C.MESHES["254" if ci else "rcr22"](w, h)
        lab = R.labels(t, tri, w, h)
        assert (lab == R.NONE).any()
        x = C.rows_for(frames, C.ROWS, idx, t, w, h, C.SEED)
        fitted = R.matrices(x, idx, t, tri)
        for r, im in enumerate(C.ROWS):
            f = dict(frames[im])
            if ci:
                f["fmt"] = swapped.get(f["fmt"], f["fmt"])                    # the same bytes as RGB and BGRA: all six formats
            b0, b1 = K.plane_bytes(f)
            planes = (buf[f["off"]:f["off"] + b0].tobytes(), buf[f["uv_off"]:f["uv_off"] + b1].tobytes() if b1 else b"")
            host = K.host_frame(buf, f)
            for mats, filt in ((fitted[r], (1, 16, 1.0)), (fitted[r], (1, 3, 2.0)), (border_matrices(f, w, h, len(tri)), (1, 16, 1.0))) + \
                              (((fitted[r], (0, 16, 1.0)),) if r == 3 else ()):
                add(planes, f, host, mats, lab, w, h, filt)
    assert seen == set(range(6))
    assert len({p[1:] for p in pairs}) >= 8 and all(any(p[0] == fmt and p[1] != p[2] for p in pairs) for fmt in range(6))
    # ---- the accumulator bound: one triangle at 16 x on an all-255 gray frame
    w, h = C.CROPS[0]
    idx, t, tri = C.MESHES["single"](w, h)
    lab1 = R.labels(t, tri, w, h)
    white = dict(fmt=T.GRAY, w=400, h=340, stride=400, off=0, uv_off=None)
    m16 = np.array([[16, 0, 8, 0, 16, 8]], f32)
    add((bytes([255]) * (400 * 340), b""), white, T.Frame(T.GRAY, np.full((340, 400), 255, np.uint8)), m16, lab1, w, h, (1, 16, 1.0))
    blob[0] = struct.pack("<i", len(cases))
    (tmp_path / "cases.bin").write_bytes(b"".join(head) + b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 600, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at = 8 * len(rules)
    assert np.array_equal(got[:at].view(np.int32).reshape(-1, 2), want_rules)
    tops = []
    for frame, mats, lab, S in cases:
        h, w = lab.shape
        assert np.array_equal(got[at:at + 8 * len(S)].view(np.int32).reshape(-1, 2), S)
        at += 8 * len(S)
        kind, bgr, y = WA.warped(frame, mats, lab, S)
        n = w * h
        assert np.array_equal(got[at:at + 3 * n].reshape(h, w, 3), bgr), (frame.fmt, frame.w, frame.h, w, h)
        assert not bgr[lab == R.NONE].any()
        at += 3 * n
        for shift in (14, 15):
            want = T.finish(kind, bgr, y, "uint8", "nhwc", 1, "bgr", gray_shift=shift)[..., 0]
            assert np.array_equal(got[at:at + n].reshape(h, w), want), (frame.fmt, shift)
            at += n
        want = T.finish(kind, bgr, None, "float32", "nchw", 3, "rgb", scale, bias)
        assert np.array_equal(got[at:at + 12 * n].copy().view(np.uint32).reshape(3, h, w), want.view(np.uint32)), frame.fmt
        at += 12 * n
        tops.append(int(got[at:at + 4].view(np.uint32)[0]))
        at += 4
    assert at == got.size
    # the bound case: Sx = Sy = 16, every sub-sample of every labelled pixel inside the frame, the sum exactly at its largest value
    frame, mats, lab, S = cases[-1]
    assert tuple(S[0]) == (16, 16) and tops[-1] == 255 * 1024 * 256 + 512 * 256 and tops[-1] < 2 ** 26 + 2 ** 17
    assert max(tops) == tops[-1]
    assert (WA.warped(frame, mats, lab, S)[1][lab != R.NONE] == 255).all()
