"""sdm_align_region_mask without a device: the kernels' arithmetic compiled for the host (tests/cpp/region_mask_host.cpp, address and
undefined-behaviour sanitizers, every point list, workspace and map in a heap block of exactly its bytes) against the numpy restatement
(tests/region_mask_ref.py), bit for bit on the maps, the hulls' vertex lists and the flags; the contract's two check values; the Python
layer's argument errors and preset resolution."""
import ctypes
import struct

import numpy as np
import pytest

import align_ref as A
import cpp_build as B
import region_mask_cases as C
import region_mask_ref as R
from superviseddescent_amd import _lib, ibug

f32 = np.float32
FLAGGED = [                                                              # rows that draw nothing, appended to the triangle group
    (C.IDENTITY, np.array([[2.0e6, 0], [0, 0], [0, 5]], f32), R.NONFINITE),
    (C.IDENTITY, np.array([[1, 1], [np.nan, 0], [0, 5]], f32), R.NONFINITE),
    (C.IDENTITY, np.array([[1, 1], [5, np.inf], [0, 5]], f32), R.NONFINITE),
    (np.array([1, 2, 0, 2, 4, 0], f32), np.array([[1, 1], [5, 0], [0, 5]], f32), A.DEGENERATE),
    (np.array([1, 0, np.nan, 0, 1, 0], f32), np.array([[1, 1], [5, 0], [0, 5]], f32), A.DEGENERATE),
]


def test_check_value_square():
    """the square (2,2) (9,2) (9,9) (2,9) in a 12 x 12 crop at grow 0, feather 0"""
    sq = np.array([[2, 2], [9, 2], [9, 9], [2, 9]], f32)
    m = R.rasterise([sq], 0, 12, 12)
    want = np.zeros((12, 12), np.uint8)
    want[2:10, 2:10] = 128
    want[3:9, 3:9] = 255
    assert np.array_equal(m, want)
    assert np.array_equal(R.rasterise([sq[::-1]], 0, 12, 12), want)      # the orientation does not matter


def test_check_value_bow_tie():
    """the bow-tie (2,2) (14,12) (14,2) (2,12): both lobes filled (non-zero winding), 128 at the crossing pixel (8, 7)"""
    bow = np.array([[2, 2], [14, 12], [14, 2], [2, 12]], f32)
    m = R.rasterise([bow], 0, 17, 15)
    assert m[7, 8] == 128
    assert m[7, 4] == 255 and m[7, 12] == 255                            # left and right lobe
    assert m[3, 8] == 0 and m[11, 8] == 0 and m[0, 0] == 0               # above and below the crossing: outside


def test_hull_rules():
    pts = np.array([[0, 0], [2, 0], [1, 0], [2, 2], [0, 2], [1, 1], [2, 0], [1, 2], [0, 1]], f32)
    assert R.hull(pts).tolist() == [[0, 0], [2, 0], [2, 2], [0, 2]]      # duplicates and collinear points dropped; lower, then upper chain
    assert R.hull(np.array([[3, 1], [1, 1], [2, 1]], f32)).tolist() == [[1, 1], [3, 1]]
    assert R.hull(np.array([[3, 1]] * 4, f32)).tolist() == [[3, 1]]
    assert R.turn((0, 0), (1, 0), (1, 1)) == 1 and R.turn((0, 0), (1, 1), (1, 0)) == -1 and R.turn((0, 0), (1, 1), (2, 2)) == 0
    # a one-vertex and a two-vertex polygon: the distance to the point / the segment, never inside
    one = R.rasterise([np.array([[4, 4]], f32)], 0, 9, 9, grow=2.0)
    assert one[4, 4] == 255 and one[4, 6] == 128 and one[4, 7] == 0
    two = R.rasterise([np.array([[2, 4], [6, 4]], f32)], 0, 9, 9)
    assert two[4, 2:7].tolist() == [128] * 5 and two[3, 4] == 0


def test_feather_and_grow_move_the_ramp():
    sq = [np.array([[4, 4], [27, 4], [27, 27], [4, 27]], f32)]
    a = R.rasterise(sq, 0, 32, 32, grow=0.0, feather=8.0)[16]
    assert a[4] == 128 and a[0] == 0 and a[8] == 255 and (np.diff(a[:9].astype(int)) > 0).all()
    b = R.rasterise(sq, 0, 32, 32, grow=2.0, feather=8.0)[16]
    assert b[2] == 128 and np.array_equal(b[:14], a[2:16]) and np.array_equal(b[18:], a[16:-2])       # both ramps moved outwards by two pixels
    assert R.rasterise(sq, 0, 32, 32, grow=-3.0)[16, 7] == 128


def host_cases():
    """every group of region_mask_cases at four crop sizes, the parameter sets in turn; the flagged rows ride with the triangles"""
    cases, k = [], 0
    for (w, h) in [(1, 1), (5, 7), (16, 16), (37, 29)]:
        for name, sizes, nh, bits, rows in C.groups(w, h):
            grow, feather = C.PARAMS[k % len(C.PARAMS)]
            k += 1
            extra = [(M, p) for M, p, _ in FLAGGED] if name == "triangle" else []
            cases.append(dict(w=w, h=h, name=name, sizes=sizes, nh=nh, bits=bits, rows=list(rows) + extra, grow=grow, feather=feather))
    return cases


def test_host_build_of_the_arithmetic_under_sanitizers(tmp_path):
    exe = B.host_program("region_mask_host", tmp_path)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for c in cases:
        blob.append(struct.pack("<5i2f", c["w"], c["h"], len(c["sizes"]), c["nh"], c["bits"], c["grow"], c["feather"])
                    + struct.pack(f"<{len(c['sizes'])}i", *c["sizes"]) + struct.pack("<i", len(c["rows"])))
        for M, p in c["rows"]:
            p = np.ascontiguousarray(p, f32)
            blob.append(np.asarray(M, f32).tobytes() + struct.pack("<i", p.nbytes) + p.tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at, seen, lit, short = 0, 0, 0, set()
    for c in cases:
        w, h, G = c["w"], c["h"], len(c["sizes"])
        for r, (M, p) in enumerate(c["rows"]):
            want, wflags, polys = R.mask_row(M, p, c["sizes"], c["nh"], c["bits"], w, h, c["grow"], c["feather"])
            flags = int(got[at:at + 4].view(np.int32)[0]); at += 4
            counts = got[at:at + 4 * G].view(np.int32); at += 4 * G
            assert flags == wflags, (c["name"], w, h, r)
            assert counts.tolist() == ([0] * G if polys is None else [len(q) for q in polys]), (c["name"], w, h, r)
            for g in range(G if polys is not None else 0):
                v = got[at:at + 8 * counts[g]].view(np.uint32); at += 8 * counts[g]
                assert np.array_equal(v, polys[g].reshape(-1).view(np.uint32)), (c["name"], w, h, r, g)
                if c["bits"] >> g & 1:
                    short.add(min(int(counts[g]), 3))
            m = got[at:at + w * h].reshape(h, w); at += w * h
            assert np.array_equal(m, want), (c["name"], w, h, r, c["grow"], c["feather"])
            seen |= flags | (int(flags == 0) << 8)
            lit += int((m > 0).sum())
    assert at == got.size
    assert seen == 0x100 | A.DEGENERATE | R.NONFINITE and lit > 5000 and short == {1, 2, 3}          # hulls of one, two and more vertices


def test_flagged_rows_of_the_restatement():
    for M, p, flag in FLAGGED:
        m, f, polys = R.mask_row(M, p, [3], width=8, height=8)
        assert f == flag and not m.any() and polys is None


def test_symbols_struct_and_constants():
    assert {"sdm_align_region_mask", "sdm_align_region_mask_at"} <= set(_lib.EXPORTED)
    assert _lib.SDM_REGION_NONFINITE == 16 == R.NONFINITE
    assert ctypes.sizeof(_lib.SdmRegionMask) == 32
    region, keep = _lib.region_mask([27, 12, 4], 1, hull=(0, 2), grow=2.5, feather=4)
    assert (region.n_polygons, region.n_holes, region.hull_bits, region.grow, region.feather) == (3, 1, 5, 2.5, 4.0)
    assert [region.sizes[g] for g in range(3)] == [27, 12, 4]
    for bad in (dict(sizes=[]), dict(sizes=[3] * 9), dict(sizes=[3], hull=(1,)), dict(sizes=[3, 3], hull=(-1,))):
        with pytest.raises(ValueError):
            _lib.region_mask(**bad)


def test_presets_resolve_against_the_model():
    face68 = ibug.region_preset("face", ibug.IBUG68_IDS)
    assert face68[:3] == ["1", "2", "3"] and face68[16:19] == ["17", "27", "26"] and face68[-1] == "18" and len(face68) == 27
    assert ibug.region_preset("face", ibug.RCR22_IDS) == ("hull", ibug.RCR22_IDS)
    assert ibug.region_preset("mouth_outer", ibug.RCR22_IDS) == ["49", "52", "55", "58"]
    assert len(ibug.region_preset("mouth_outer", ibug.IBUG68_IDS)) == 12
    assert ibug.region_preset("right_eye", ibug.RCR22_IDS) == [str(i) for i in range(37, 43)]
    for name in ibug.REGIONS:
        assert all(i in ibug.IBUG68_IDS for i in ibug.region_preset(name, ibug.IBUG68_IDS))
    for name, region in ibug.REGIONS_RCR22.items():
        assert all(i in ibug.RCR22_IDS for i in (region[1] if isinstance(region, tuple) else region))
    with pytest.raises(ValueError, match="'28'"):
        ibug.region_preset("nose", ibug.RCR22_IDS)                       # RCR-22 lacks the bridge of the nose
    with pytest.raises(ValueError, match="needs landmark ids"):
        ibug.region_preset("mouth_inner", ibug.RCR22_IDS)
    with pytest.raises(ValueError, match="unknown region"):
        ibug.region_preset("chin", ibug.IBUG68_IDS)
    with pytest.raises(ValueError, match="lacks"):
        ibug.region_preset("face", ["1", "2", "3"])


def test_detection_model_region_index():
    """names, ("hull", ids) and presets to landmark positions, the holes behind the regions; no device is touched"""
    from superviseddescent_amd import detection_model
    dm = detection_model.__new__(detection_model)
    dm.landmark_ids = list(ibug.RCR22_IDS)
    polys, holes, hull = dm._region_index(["face", ["37", "40", "43"]], ["mouth_outer", ("hull", ["37", "38", "39", "40"])])
    pos = dm.landmark_ids.index
    assert polys == [list(range(22)), [pos("37"), pos("40"), pos("43")]]
    assert holes == [[pos(i) for i in ("49", "52", "55", "58")], [pos(i) for i in ("37", "38", "39", "40")]]
    assert hull == [0, 3]
    assert dm._region_index("face", ())[2] == [0] and dm._region_index(("hull", ["37", "40", "43"]), "right_eye")[1] == [[pos(str(i)) for i in range(37, 43)]]
    with pytest.raises(ValueError, match="not in this model"):
        dm._region_index([["1", "2", "3"]], ())
    with pytest.raises(ValueError, match="lacks"):
        dm._region_index(["nose"], ())
