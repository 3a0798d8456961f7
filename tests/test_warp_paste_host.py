"""sdm_warp_paste_tensor without a device: properties of the numpy restatement alone (tests/warp_paste_ref.py) against exact rational
geometry; feather_warp_mask; and the kernels' per-row, per-triangle and per-pixel code compiled for the host
(tests/cpp/warp_paste_host.cpp, address and undefined-behaviour sanitizers, every frame, tensor, label map and opacity map in a heap
block of exactly its bytes, run as a child process) against the restatement, bit for bit: the flags, every A_t and W_t, the row boxes
and every byte the frame owns, with the rows pasted in descending and in ascending order.  The host program walks pixels in plain
loops; the kernel's wave-wide cull and its LDS staging run only in tests/test_gpu_warp_paste.py."""
import itertools
import struct
from fractions import Fraction

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import paste_cases as C
import warp_cases as WC
import warp_paste_ref as WP
import warp_ref as R
from superviseddescent_amd import _lib, feather_warp_mask

f32 = np.float32
COMBOS = list(itertools.product(("uint8", "float16", "float32"), ("nhwc", "nchw"), (1, 3), ("bgr", "rgb")))
MESHES = (WC.mesh_rcr22, WC.mesh_single, WC.mesh_254)


def placed(template, S, rng, noise=0.4):
    """K x 2 float32: the template seen through the crop -> frame similarity S, every landmark moved by up to `noise` pixels"""
    t = np.asarray(template, np.float64)
    return (t @ S[:, :2].T + S[:, 2] + rng.uniform(-noise, noise, t.shape)).astype(f32)


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def exactly_inside(p, tri, X, Y):
    """strictly inside triangle tri of the float32 points p, in rational arithmetic"""
    a, b, c = ([Fraction(float(v)) for v in p[i]] for i in tri)
    e = [(r[0] - q[0]) * (Y - q[1]) - (r[1] - q[1]) * (X - q[0]) for q, r in ((a, b), (b, c), (c, a))]
    return all(v > 0 for v in e) or all(v < 0 for v in e)


def test_no_cracks_in_a_mesh_that_does_not_fold():
    W, H = 30, 26
    _, t, tri = WC.mesh_rcr22(24, 20)
    rng = np.random.default_rng(3)
    for S in (np.array([[1.1, 0.2, 2.0], [-0.2, 1.1, 4.0]]), np.array([[0.6, -0.5, 12.0], [0.5, 0.6, 1.0]])):
        p = placed(t, S, rng, 0.03)                                            # (gentle enough that not even the mesh's slivers fold)
        assert WP.flags(p, t, tri, [(W, H)])[0] & WP.FOLDED == 0
        tmap = WP.triangle_map(p, tri, WP.matrices(p, t, tri)[0], W, H)
        n_inside = 0
        for Y in range(H):
            for X in range(W):
                if any(exactly_inside(p, tr, X, Y) for tr in tri):
                    n_inside += 1
                    assert tmap[Y, X] >= 0 and exactly_inside_or_on(p, tri[tmap[Y, X]], X, Y), (X, Y)
        assert n_inside > 50


def exactly_inside_or_on(p, tri, X, Y):
    a, b, c = ([Fraction(float(v)) for v in p[i]] for i in tri)
    e = [(r[0] - q[0]) * (Y - q[1]) - (r[1] - q[1]) * (X - q[0]) for q, r in ((a, b), (b, c), (c, a))]
    return all(v >= 0 for v in e) or all(v <= 0 for v in e)


SQUARE = np.array([[1, 1], [9, 1], [9, 9], [1, 9]], f32)         # two triangles that share the diagonal (1, 1) - (9, 9)
SQUARE_T = np.array([[2, 2], [14, 2], [14, 14], [2, 14]], f32)


def test_a_pixel_on_a_shared_edge_gets_the_lower_index():
    for tri in (np.array([[0, 1, 2], [0, 2, 3]]), np.array([[0, 2, 3], [0, 1, 2]]), np.array([[0, 2, 1], [0, 2, 3]])):
        tmap = WP.triangle_map(SQUARE, tri, WP.matrices(SQUARE, SQUARE_T, tri)[0], 12, 12)
        assert [tmap[i, i] for i in range(1, 10)] == [0] * 9                  # the diagonal, corners included
        assert tmap[2, 8] == (0 if 1 in tri[0] else 1) and tmap[8, 2] == (1 if 1 in tri[0] else 0)
        assert (tmap[1:10, 1:10] >= 0).all() and (tmap >= 0).sum() == 81


def test_a_triangle_without_area_covers_nothing_and_leaves_its_neighbours():
    tri = np.array([[0, 1, 4], [0, 1, 2], [0, 2, 3]])
    p = np.concatenate([SQUARE, [[5, 1]]]).astype(f32)                         # landmark 4 on the edge 0 - 1: triangle 0 is flat
    t = np.concatenate([SQUARE_T, [[8, 5]]]).astype(f32)
    tmap = WP.triangle_map(p, tri, WP.matrices(p, t, tri)[0], 12, 12)
    both = WP.triangle_map(SQUARE, tri[1:], WP.matrices(SQUARE, SQUARE_T, tri[1:])[0], 12, 12)
    assert WP.det_e(p, tri)[0] == 0 and not (tmap == 0).any()
    assert np.array_equal(tmap, np.where(both >= 0, both + 1, -1))
    assert WP.flags(p, t, tri, [(12, 12)])[0] == WP.FOLDED


def test_a_mirrored_triangle_still_pastes():
    tri = np.array([[0, 1, 2]])
    t = SQUARE_T[:3]
    p = SQUARE[[0, 2, 1]]                                                      # b and c exchanged: det E < 0 against D > 0
    assert WP.flags(p, t, tri, [(12, 12)])[0] == WP.FOLDED
    mats = WP.matrices(p, t, tri)[0]
    lab = R.labels(t, tri, 16, 16)
    pix = np.zeros((12, 12, 1), np.uint8)
    foot, a, tmap = WP.paste_row(pix, T.GRAY, p, tri, mats, lab, np.full((1, 16, 16), 200, np.uint8), channels=1)
    same = WP.triangle_map(SQUARE[:3], tri, WP.matrices(SQUARE[:3], t, tri)[0], 12, 12)
    assert np.array_equal(tmap, same) and (tmap == 0).sum() == 45
    assert foot.sum() == 45 and (pix[..., 0] == 200).sum() >= 28 and (pix > 0).sum() > 36


def test_the_box_holds_every_pixel_that_has_a_triangle():
    rng = np.random.default_rng(11)
    for mesh, (cw, ch) in itertools.product(MESHES, WC.CROPS):
        _, t, tri = mesh(cw, ch)
        for r in range(4):
            S = K.similarities([dict(w=40, h=36)], [0] * 4, cw, ch, 50 + r)[r]
            p = placed(t, S, rng)
            full = WP.triangle_map(p, tri, WP.matrices(p, t, tri)[0], 40, 36, use_box=False)
            x0, y0, x1, y1 = WP.box(p, 40, 36)
            ys, xs = np.nonzero(full >= 0)
            assert ys.size == 0 or (x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1)
            assert np.array_equal(full, WP.triangle_map(p, tri, WP.matrices(p, t, tri)[0], 40, 36))


# ---- feather_warp_mask -------------------------------------------------------------------------------------------------------------
def test_feather_warp_mask():
    _, t, tri = WC.mesh_rcr22(33, 17)
    m = R.labels(t, tri, 33, 17) != R.NONE
    for radius in (0, 1, 3):
        a = feather_warp_mask(m, radius)
        assert a.dtype == np.uint8 and a.shape == m.shape and np.array_equal(a == 0, ~m)          # 0 exactly on unlabelled pixels
        if radius == 0:
            assert np.array_equal(a, 255 * m.astype(np.uint8))
    a = feather_warp_mask(m, 3).astype(int)
    # monotone towards the inside: a pixel is at most one step above its lowest neighbour (the crop's outside counts as 0)
    pad = np.pad(a, 1)
    low = np.minimum(np.minimum(pad[:-2, 1:-1], pad[2:, 1:-1]), np.minimum(pad[1:-1, :-2], pad[1:-1, 2:]))
    assert (a >= low).all() and (a <= low + 64).all() and a.max() == 255
    sym = np.zeros((9, 11), bool)
    sym[2:7, 1:10] = True
    s = feather_warp_mask(sym, 2)
    assert np.array_equal(s, s[::-1]) and np.array_equal(s, s[:, ::-1]) and s[4, 5] == 255 and s[2, 1] == 85 and s[3, 2] == 170
    assert feather_warp_mask(np.ones((3, 5), bool), 1).tolist() == [[128] * 5, [128, 255, 255, 255, 128], [128] * 5]
    with pytest.raises(ValueError):
        feather_warp_mask(m, -1)
    assert {"sdm_warp_paste_tensor", "sdm_warp_paste_tensor_at"} <= set(_lib.EXPORTED)


# ---- the host build of the kernels' code -------------------------------------------------------------------------------------------
def special_rows(base, tri, f):
    """beyond the similarities: wholly outside the frame, a NaN landmark, a flat triangle, a folded one, landmarks of 1e30"""
    a, b, c = tri[0]
    out = base + np.array([f["w"] + 60.0, -90.0], f32)
    nan = base.copy(); nan[b, 1] = np.nan
    flat = np.rint(base).astype(f32); flat[c] = flat[a] + 2 * (flat[b] - flat[a])          # c on the line a - b, exactly
    fold = base.copy(); fold[[b, c]] = fold[[c, b]]
    far = base.copy(); far[a] = (1e30, -1e30)
    return [out, nan, flat, fold, far]


def host_cases():
    """one frame with eight rows per case: three meshes x two crops x the seven frames of tests/paste_cases.py (1 x 1 and 2 x 2 up to
    131 x 7, the five formats)"""
    buf, frames = C.place(C.FRAMES, 5)
    cases = []
    for mesh, (cw, ch), (i, f) in itertools.product(MESHES, WC.CROPS, enumerate(frames)):
        k = len(cases)
        rng = np.random.default_rng(400 + k)
        _, t, tri = mesh(cw, ch)
        dtype, layout, channels, order = COMBOS[(5 * k) % len(COMBOS)]
        pts = [placed(t, S, rng) for S in K.similarities(frames, [i] * 3, cw, ch, 100 + k)]
        pts += special_rows(pts[2], tri, f)
        mode = k % 3
        x = C.tensor(len(pts), cw, ch, dtype, layout, channels, 200 + k)
        alpha = None if mode == 0 else C.alpha_maps(1 if mode == 1 else len(pts), cw, ch, 300 + k, zero_band=k % 2 == 1)
        cases.append(dict(f=f, cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14 + k % 2,
                          pts=np.stack(pts), t=t, tri=np.asarray(tri, np.int32), lab=R.labels(t, tri, cw, ch), x=x, alpha=alpha, mode=mode,
                          frame=buf[f["off"]:f["off"] + C.owned_bytes(f)].copy()))
    return cases + needle_cases(buf, frames, len(cases))


# one far landmark per row -- (landmark, (x, y)) -- under which a triangle of the RCR-22 mesh that is NOT skipped (d != 0, W_t finite) has
# rounded edge functions >= 0 beyond its corners' box, found by a search over the restatement; the rows of 1e9 and 1e12 complete the range
FAR = {(37, 29): [(10, (3.5825050345464083e+17, 3.58239332425521e+17)), (7, (3.764387911153937e+18, -8.540806216665226e+17)),
                  (11, (9.900501726927255e+17, -2.6032714226526787e+17)), (2, (4.4367484694929816e+16, -9.705770454709618e+17)),
                  (17, (1.3107842412616768e+17, -1.3106899231475907e+17)), (5, (1e9, -1e9)), (9, (-1e12, 3e12))],
       (64, 48): [(13, (8.179777194458742e+17, -8.179014247085851e+17)), (3, (-6.64046515388771e+17, 6.640328288501615e+17)),
                  (15, (6.439657211162653e+17, -6.439635473815441e+17)), (18, (2.518092302178357e+17, -2.5179869338943907e+17)),
                  (1, (-1.1228733862939558e+18, 1.4052289812635606e+17)), (5, (1e9, -1e9)), (9, (-1e12, 3e12))],
       (48, 40): [(15, (2.995554320410157e+17, 2.9954043286442714e+17)), (16, (5.4138581579288736e+17, -5.4136298172972806e+17)),
                  (7, (-1.2692662138246572e+18, 4.7130947766668115e+17)), (3, (8.473466455559818e+17, 8.472644512739875e+17)),
                  (5, (1e9, -1e9))]}


def spanning_rows(t, fw, fh, cw, ch, n, rng):
    """n rows of K x 2 float32 that all span an fw x fh frame: the first len(FAR[fw, fh]) are the template stretched over the frame
    with one landmark of FAR, the others the same with every landmark moved by up to 1.5 pixels"""
    span = np.array([[1.2 * fw / cw, 0.1, -0.1 * fw], [-0.1, 1.2 * fh / ch, -0.1 * fh]])
    far = FAR[fw, fh]
    pts = [placed(t, span, rng, 0.0 if r < len(far) else 1.5) for r in range(n)]
    for row, (j, xy) in zip(pts, far):
        row[j] = xy
    return np.stack(pts)


def needle_cases(buf, frames, k0):
    """the 37 x 29 BGR and the 64 x 48 RGBA frame under eight rows of the RCR-22 mesh that all span the frame and lie over one another,
    seven of them with one landmark at a large finite distance (1e9 ... 4e18): the triangles at that landmark are needles whose
    rounded edge functions are >= 0 many pixels beyond their corners, where only the triangle's box decides"""
    cases = []
    for i, (cw, ch) in zip((0, 1), WC.CROPS):
        k, f = k0 + len(cases), frames[i]
        _, t, tri = WC.mesh_rcr22(cw, ch)
        pts = spanning_rows(t, f["w"], f["h"], cw, ch, 8, np.random.default_rng(400 + k))
        dtype, layout, channels, order = COMBOS[(5 * k) % len(COMBOS)]
        x = C.tensor(8, cw, ch, dtype, layout, channels, 200 + k)
        alpha = np.full((1, ch, cw), 128, np.uint8)
        cases.append(dict(f=f, cw=cw, ch=ch, dtype=dtype, layout=layout, channels=channels, order=order, gray_shift=14 + k % 2,
                          pts=pts, t=t, tri=np.asarray(tri, np.int32), lab=R.labels(t, tri, cw, ch), x=x, alpha=alpha, mode=1,
                          frame=buf[f["off"]:f["off"] + C.owned_bytes(f)].copy(), needle=True))
    return cases


def test_host_build_of_the_pixel_code_under_sanitizers(tmp_path):
    exe = B.host_program("warp_paste_host", tmp_path)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        G, qa, D = R.constants(c["t"], c["tri"])
        consts = np.concatenate([G.reshape(-1, 4), qa, D[:, None]], 1).astype(np.float64)
        blob.append(struct.pack("<15i", f["fmt"], f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["pts"]),
                                c["mode"], c["t"].shape[0], c["tri"].shape[0])
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + c["tri"].tobytes() + consts.tobytes() + c["pts"].astype(f32).tobytes()
                    + struct.pack("<i", c["lab"].size) + c["lab"].tobytes()
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + struct.pack("<i", c["frame"].size) + c["frame"].tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 120, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at, seen, touched, boxed, formats = 0, 0, 0, 0, set()
    for k, c in enumerate(cases):
        f, n, Tn = c["f"], len(c["pts"]), c["tri"].shape[0]
        flags = got[at:at + 4 * n].view(np.int32); at += 4 * n
        A = got[at:at + 24 * n * Tn].view(f32).reshape(n, Tn, 6); at += 24 * n * Tn
        Wt = got[at:at + 24 * n * Tn].view(f32).reshape(n, Tn, 6); at += 24 * n * Tn
        cov = got[at:at + 4 * n * Tn].view(np.int32).reshape(n, Tn); at += 4 * n * Tn
        box = got[at:at + 16 * n].view(np.int32).reshape(n, 4); at += 16 * n
        frame = got[at:at + c["frame"].size]; at += c["frame"].size          # rows pasted in descending order
        ascending = got[at:at + c["frame"].size]; at += c["frame"].size
        mats = WP.matrices(c["pts"], c["t"], c["tri"])
        assert np.array_equal(flags, WP.flags(c["pts"], c["t"], c["tri"], [(f["w"], f["h"])] * n)), k
        for r in range(n):
            if flags[r] & WP.DEGENERATE:                                        # (NaN, whatever its sign and payload)
                assert np.isnan(A[r]).all() and np.isnan(mats[r]).all(), (k, r)
            else:
                assert np.array_equal(A[r].view(np.uint32), mats[r].view(np.uint32)), (k, r)
            assert box[r].tolist() == list(WP.box(c["pts"][r], f["w"], f["h"])), (k, r)
            if flags[r] & WP.DEGENERATE or box[r, 2] == 0:
                assert not cov[r].any()
                continue
            W_ref, skipped = WP.inverses(mats[r])
            assert np.array_equal(Wt[r][~skipped].view(np.uint32), W_ref[~skipped].view(np.uint32)), (k, r)
            assert np.array_equal(cov[r] != 0, ~skipped & ~(WP.det_e(c["pts"][r], c["tri"]) == 0)), (k, r)
        want = c["frame"].copy()
        pix = C.view(want, dict(f, off=0))
        rows = [(c["pts"][r], mats[r], c["x"][r], None if c["alpha"] is None else c["alpha"][r if c["mode"] == 2 else 0]) for r in range(n)]
        WP.paste(pix, f["fmt"], rows, c["tri"], c["lab"], layout=c["layout"], channels=c["channels"], order=c["order"], scale=C.SCALES,
                 bias=C.BIASES, gray_shift=c["gray_shift"])
        assert np.array_equal(frame, want), (k, f, c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"])
        assert np.array_equal(ascending, want), (k, f)
        if c.get("needle"):
            # the triangle's box decides here: without it the edge functions alone give other triangles to some pixels of the frame
            for r in range(n):
                with_box = WP.triangle_map(c["pts"][r], c["tri"], mats[r], f["w"], f["h"])
                boxed += int((with_box != WP.triangle_map(c["pts"][r], c["tri"], mats[r], f["w"], f["h"], tri_box=False)).sum())
        seen |= int(np.bitwise_or.reduce(flags)) | (int(flags.min() == 0) << 8)
        touched += int((want != c["frame"]).sum())
        formats.add(f["fmt"])
    assert at == got.size
    assert seen == 0x100 | WP.DEGENERATE | WP.PARTIAL | WP.FOLDED and touched > 10000, (hex(seen), touched)
    assert formats == {T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA}
    assert boxed > 500, "hardly a pixel of the needle cases was decided by a triangle's box"
