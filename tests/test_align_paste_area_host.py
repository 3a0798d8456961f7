"""sdm_align_paste_tensor_filtered without a device: the kernel's per-pixel code and its prepare stage compiled for the host
(tests/cpp/align_paste_area_host.cpp, address and undefined-behaviour sanitizers, every frame, tensor and opacity map in a heap block of
exactly its bytes) against the numpy restatement (tests/paste_area_ref.py), bit for bit on every byte the frame owns; that the working
footprint and the box hold every pixel the formula touches; a known answer that needs neither implementation; the aliasing the filter
is for; the choice of S; the Python argument handling."""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import align_ref as A
import align_area_ref as R
import align_tensor_ref as T
import cpp_build as B
import paste_area_cases as D
import paste_area_ref as Q
import paste_cases as C
import paste_ref as P
from superviseddescent_amd import _lib

f32 = np.float32
SPEC = ("layout", "channels", "order", "gray_shift")


def plain_case(fmt, pix, cw, ch, mats, x, filt=(Q.AREA, 16, 1.0), channels=1):
    """a case on a dense frame `pix` (H x W x bpp), a uint8 NHWC tensor, no opacity map"""
    h, w, bpp = pix.shape
    return dict(f=dict(fmt=fmt, w=w, h=h, stride=w * bpp), cw=cw, ch=ch, dtype="uint8", layout="nhwc", channels=channels, order="bgr",
                gray_shift=14, mats=[np.asarray(m, f32) for m in mats], x=np.ascontiguousarray(x), alpha=None, mode=0, filter=filt,
                frame=pix.reshape(-1).copy())


def next_above_four():
    """a matrix whose float32 W has s2 = W00 W00 + W10 W10 equal to the float32 next above 4.0"""
    target = np.nextafter(f32(4.0), f32(8.0))
    for w in np.linspace(5.0e-4, 9.0e-4, 4001):
        M = (np.array([[2.0, w, 0.0], [-w, 2.0, 0.0]]) / (4.0 + w * w)).astype(f32)
        if Q.s2_of(M) == target:
            return M
    raise AssertionError("no matrix found")


def selection_case():
    mats = [np.array([[0.5, 0, 1], [0, 0.5, 1]], f32), next_above_four(), np.array([[1e-20, 0, 3], [0, 1e-20, 3]], f32),
            np.array([[1, 0, np.nan], [0, 1, 0]], f32), np.array([[0.125, 0, 2], [0, 0.125, 2]], f32),
            np.array([[5e-6, 0, 3], [0, 5e-6, 3]], f32)]            # W00 = 2e5: beyond the reach the footprint claims, the box alone decides
    x = np.random.default_rng(3).integers(0, 256, (len(mats), 16, 16, 1), dtype=np.uint8)
    return plain_case(T.BGR, np.zeros((8, 8, 3), np.uint8), 16, 16, mats, x)


def extra_cases():
    """behind the cases of paste_area_cases.host_cases: the known answer, the two checkerboards, the S selection"""
    M, crop, _, _ = D.known_answer()
    out = [plain_case(T.BGR, np.zeros((8, 8, 3), np.uint8), 16, 16, [M], crop[None, :, :, None])]
    for theta in (0.0, 0.3):
        M, crop, frame, _ = D.checkerboard(theta)
        out.append(plain_case(T.BGR, frame, 64, 64, [M], crop[None, :, :, None]))
    return out + [selection_case()]


def restate(c):
    """(the frame's bytes after the restatement, [(S, a)] per row); a degenerate row pastes nothing"""
    want = c["frame"].copy()
    pix = C.view(want, dict(c["f"], off=0))
    mode, cap, gate = c["filter"]
    res = []
    for r, m in enumerate(c["mats"]):
        if P.inverse(m)[1]:
            res.append((1, np.zeros(pix.shape[:2], np.int64)))
            continue
        S = Q.samples(m, mode, cap, gate)
        a = None if c["alpha"] is None else c["alpha"][r if c["mode"] == 2 else 0]
        res.append((S, Q.paste_row(pix, c["f"]["fmt"], m, c["x"][r], a, S, scale=C.SCALES, bias=C.BIASES, **{k: c[k] for k in SPEC})))
    return want, res


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    """the host program built under the sanitizers and run ONCE, as a child process, on every case: [(case, its output)]"""
    tmp = tmp_path_factory.mktemp("paste_area")
    exe = B.host_program("align_paste_area_host", tmp)
    cases = D.host_cases() + extra_cases()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        f = c["f"]
        a = b"" if c["alpha"] is None else c["alpha"].tobytes()
        blob.append(struct.pack("<15if", f["fmt"], f["w"], f["h"], f["stride"], c["cw"], c["ch"], _lib.ALIGN_DTYPES[c["dtype"]],
                                _lib.ALIGN_LAYOUTS[c["layout"]], c["channels"], _lib.ALIGN_ORDERS[c["order"]], c["gray_shift"], len(c["mats"]),
                                c["mode"], c["filter"][0], c["filter"][1], c["filter"][2])
                    + C.SCALES.tobytes() + C.BIASES.tobytes() + b"".join(m.tobytes() for m in c["mats"])
                    + struct.pack("<i", c["x"].nbytes) + c["x"].tobytes() + struct.pack("<i", len(a)) + a
                    + struct.pack("<i", c["frame"].size) + c["frame"].tobytes())
    (tmp / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp / "cases.bin", tmp / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp / "out.bin"), np.uint8)
    at, out = 0, []
    for c in cases:
        n, px = len(c["mats"]), c["f"]["w"] * c["f"]["h"]
        o = {}
        for name, size, view, shape in (("flags", 4 * n, np.int32, (n,)), ("W", 24 * n, np.uint32, (n, 6)), ("box", 16 * n, np.int32, (n, 4)),
                                        ("S", 4 * n, np.int32, (n,)), ("holds", n * px, np.uint8, (n, c["f"]["h"], c["f"]["w"])),
                                        ("frame", c["frame"].size, np.uint8, (-1,))):
            o[name] = got[at:at + size].view(view).reshape(shape)
            at += size
        out.append((c, o))
    assert at == got.size
    return out


def test_host_build_of_the_pixel_code_under_sanitizers(ran):
    seen, touched, formats, samples, mixed = 0, 0, set(), set(), 0
    for k, (c, o) in enumerate(ran[:-4]):
        f = c["f"]
        want, res = restate(c)
        for r, m in enumerate(c["mats"]):
            assert o["flags"][r] == P.flags_at(m, c["cw"], c["ch"], f["w"], f["h"]), (k, r)
            assert o["S"][r] == res[r][0], (k, r)
            if o["flags"][r] & A.DEGENERATE:
                assert o["S"][r] == 1 and o["box"][r].tolist() == [0, 0, 0, 0] and not o["holds"][r].any()
                continue
            assert np.array_equal(o["W"][r], P.inverse(m)[0].view(np.uint32)), (k, r)
            assert 0 <= o["box"][r, 0] <= o["box"][r, 2] <= f["w"] and 0 <= o["box"][r, 1] <= o["box"][r, 3] <= f["h"]
        assert np.array_equal(o["frame"], want), (k, f, c["cw"], c["ch"], c["dtype"], c["layout"], c["channels"], c["order"], c["filter"])
        seen |= int(o["flags"].max()) | (int(o["flags"].min() == 0) << 8)
        touched += int((want != c["frame"]).sum())
        formats.add(f["fmt"])
        if c["filter"] == (Q.AREA, 16, 1.0):
            assert o["S"][:5].tolist() == D.W_SAMPLES                       # S = 1, 2, 3, 5 and 16 (capped) on the one frame
            mixed += 1
        samples |= set(o["S"].tolist())
    assert seen == 0x100 | A.DEGENERATE | A.PARTIAL and touched > 10000 and formats == {T.GRAY, T.BGR, T.RGB, T.BGRA, T.RGBA}
    assert samples == {1, 2, 3, 4, 5, 16} and mixed >= 12


def test_footprint_and_box_hold_every_touched_pixel(ran):
    held, needed = 0, 0
    for k, (c, o) in enumerate(ran):
        _, res = restate(c)
        for r, (S, a) in enumerate(res):
            ys, xs = np.nonzero(a)
            if not ys.size:
                continue
            x0, y0, x1, y1 = o["box"][r]
            assert x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1, (k, r, S)
            assert o["holds"][r][a != 0].all(), (k, r, S)
            inside = np.zeros_like(o["holds"][r])
            inside[y0:y1, x0:x1] = 1
            assert not (o["holds"][r] & ~inside & 1).any()                   # the footprint lies in the box
            if c["alpha"] is None and ys.size >= 50:                         # (an opacity map may hold zeros inside the crop)
                held += int(o["holds"][r].sum())
                needed += ys.size
    print("pixels the formula touches", needed, "pixels the footprint holds", held)
    assert needed > 5000 and held < 2 * needed                              # ... and is no blanket over the frame


def test_known_answer(ran):
    M, crop, S, want = D.known_answer()
    c, o = ran[-4]
    assert Q.samples(M) == S and o["S"].tolist() == [S]
    pix = np.zeros((8, 8, 3), np.uint8)
    Q.paste_row(pix, T.BGR, M, crop[None], None, S, layout="nchw", channels=1)
    assert np.array_equal(pix, want) and want.any()
    assert np.array_equal(o["frame"].reshape(8, 8, 3), want)


def test_checkerboard_aliases_without_the_filter_and_not_with_it(ran):
    for (c, o), theta, bound in zip(ran[-3:-1], (0.0, 0.3), (4, 4)):
        M, crop, frame, win = D.checkerboard(theta)
        plain, area = frame.copy(), frame.copy()
        P.paste_row(plain, T.BGR, M, crop[None], None, layout="nchw", channels=1)
        S = Q.samples(M)
        Q.paste_row(area, T.BGR, M, crop[None], None, S, layout="nchw", channels=1)
        dev_plain = np.abs(plain[win].astype(int) - 128).max()
        dev_area = np.abs(area[win].astype(int) - 128).max()
        print("theta", theta, "S", S, "unfiltered deviates by", dev_plain, "area by", dev_area)
        assert S == 4 and dev_plain > 100 and dev_area <= bound
        assert o["S"].tolist() == [S] and np.array_equal(o["frame"].reshape(frame.shape), area)


def test_selection_of_S(ran):
    four, above = f32(4.0), np.nextafter(f32(4.0), f32(8.0))
    assert R.samples_of_s2(four) == 2 and R.samples_of_s2(above) == 3
    assert R.samples_of_s2(f32(30.0), max_samples=4) == 4 and R.samples_of_s2(f32(300.0)) == 16
    assert R.samples_of_s2(f32(3.9), min_scale=2.0) == 1 and R.samples_of_s2(four, min_scale=2.0) == 2
    assert R.samples_of_s2(f32(np.nan)) == 1 and R.samples_of_s2(f32(np.inf)) == 1
    assert R.samples_of_s2(f32(9.0), degenerate=True) == 1 and R.samples_of_s2(f32(9.0), mode=Q.BILINEAR) == 1
    c, o = ran[-1]
    s2 = [Q.s2_of(m) for m in c["mats"]]
    assert s2[0] == four and s2[1] == above and np.isinf(s2[2]) and s2[4] == f32(64.0)
    assert o["S"].tolist() == [2, 3, 1, 1, 8, 16] == [Q.samples(m) for m in c["mats"]]
    assert o["flags"][3] == A.DEGENERATE and not (o["flags"][[0, 1, 2, 4, 5]] & A.DEGENERATE).any()
    x0, y0, x1, y1 = o["box"][5]
    assert x1 > x0 and o["holds"][5][y0:y1, x0:x1].all() and o["holds"][5].sum() == (x1 - x0) * (y1 - y0)        # the box alone
    want, _ = restate(c)
    assert np.array_equal(o["frame"], want)
    # the cap, the gate and mode BILINEAR through the device code: the cases that carry them
    by_filter = {}
    for cc, oo in ran[:-4]:
        by_filter.setdefault(cc["filter"], []).append(oo["S"][:5].tolist())
    assert all(s == [1, 2, 3, 4, 4] for s in by_filter[(Q.AREA, 4, 1.0)])
    assert all(s == [1, 1, 3, 5, 16] for s in by_filter[(Q.AREA, 16, 2.0)])
    assert all(s == [1] * 5 for s in by_filter[(Q.BILINEAR, 16, 1.0)])


def test_mode_bilinear_and_all_rows_at_one_give_the_unfiltered_bytes(ran):
    n = 0
    for c, o in ran[:-4]:
        if (o["S"] != 1).any():
            continue
        want = c["frame"].copy()
        rows = [(m, c["x"][r], None if c["alpha"] is None else c["alpha"][r if c["mode"] == 2 else 0]) for r, m in enumerate(c["mats"])]
        P.paste(C.view(want, dict(c["f"], off=0)), c["f"]["fmt"], rows, scale=C.SCALES, bias=C.BIASES, **{k: c[k] for k in SPEC})
        assert np.array_equal(o["frame"], want)
        n += 1
    assert n >= 6


def test_symbols_structs_and_python_arguments():
    from superviseddescent_amd import Context, detection_model
    assert {"sdm_align_paste_tensor_filtered", "sdm_align_paste_tensor_at_filtered"} <= set(_lib.EXPORTED)
    assert ctypes.sizeof(_lib.SdmAlignFilter) == 12 and ctypes.sizeof(_lib.SdmAlignPaste) == 16
    for fn in (Context.align_paste_tensor, Context.align_paste_tensor_at, detection_model.paste_crops_tensor):
        p = inspect.signature(fn).parameters
        assert (p["filter"].default, p["max_samples"].default, p["min_scale"].default) == (None, 16, 1.0)
    assert Context._paste_filter(None, 16, 1.0) is None
    f = Context._paste_filter("area", 4, 2.0)
    assert (f.mode, f.max_samples, f.min_scale) == (_lib.SDM_ALIGN_FILTER_AREA, 4, 2.0)
    assert Context._paste_filter("bilinear", 16, 1.0).mode == _lib.SDM_ALIGN_FILTER_BILINEAR
    assert Context._paste_filter(f, 1, 9.0) is f
    for bad in (lambda: Context._paste_filter("lanczos", 16, 1.0), lambda: Context._paste_filter("area", 17, 1.0),
                lambda: Context._paste_filter("area", 0, 1.0), lambda: Context._paste_filter("area", 16, 0.5),
                lambda: Context._paste_filter("area", 16, float("nan")), lambda: Context._paste_filter(3, 16, 1.0)):
        with pytest.raises(ValueError):
            bad()
