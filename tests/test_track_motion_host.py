"""The tracker's motion-compensated initialisation without a device: the kernels' arithmetic (csrc/sdm_track_motion_device.h) compiled
for the host (tests/cpp/track_motion_host.cpp, address and undefined-behaviour sanitizers, every frame in a heap block of exactly its
bytes) against the numpy restatement (tests/track_motion_ref.py), bit for bit -- grids, chips, SAD tables, shifts --; the properties
of the restatement itself; the declarations of include/sdm.h, the Python argument handling and the synthetic video's new keywords."""
import hashlib
import inspect
import os
import re
import struct

import numpy as np
import pytest

import cpp_build as B
import track_motion_ref as R
from superviseddescent_amd import _lib, synth
from superviseddescent_amd.engine import Tracker

f32 = np.float32
FRAMES = [(1, 1), (5, 4), (37, 29), (64, 48)]


def pitched(img, stride):
    """the image in a block of exactly (h - 1) * stride + w bytes, the pitch bytes holding 255"""
    h, w = img.shape
    buf = np.full((h - 1) * stride + w, 255, np.uint8)
    for y in range(h):
        buf[y * stride:y * stride + w] = img[y]
    return buf


def bounds_for(k, scale, cx, cy):
    """a box whose grid has the cell size k (the cap: far beyond it) and the integer centre (cx, cy)"""
    side = 40000.0 if k == 64 else (32.0 * k - 3.0) / scale
    return cx - side / 2 + 0.25, cx + side / 2 + 0.25, cy - side / 4 + 0.5, cy + side / 4 + 0.5


def host_cases():
    """(frame stored from, frame searched, bounds, scale, S, min_gain)"""
    rng = np.random.default_rng(8086)
    cases = []
    for (w, h) in FRAMES:
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for k, S, scale in ((1, 1, 1.25), (2, 8, 0.5), (5, 16, 4.0), (64, 1, 1.25)):
            b = np.clip(a.astype(int) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
            # the chip's centre: in the frame (the chip partly outside), then far outside (wholly outside), then beyond the clamp
            for cx, cy in ((w // 2, h // 2), (w + 40 * k, -33 * k), (3.0e6, -2.5e6))[:3 if k < 64 else 1]:
                cases.append((a, b, bounds_for(k, scale, cx, cy), scale, S, int(rng.integers(0, 65))))
    a = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    cases.append((a, a[::-1].copy(), bounds_for(64, 1.0, 30, 20), 1.0, 16, 0))              # the cap with the widest search
    # a constant image, the window inside it: every SAD is equal
    flat = np.full((48, 64), 93, np.uint8)
    cases.append((flat, flat, bounds_for(1, 1.25, 32, 24), 1.25, 1, 0))
    cases.append((flat, flat, bounds_for(1, 1.25, 30, 23), 1.25, 5, 0))
    # a frame translated by exactly (3 k, -2 k), no new noise: k = 1 in 64 x 48, k = 2 in 150 x 140
    for k, (w, h), S in ((1, (64, 48), 3), (2, (150, 140), 8)):
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        b = np.zeros_like(a)
        b[:h - 2 * k, 3 * k:] = a[2 * k:, :w - 3 * k]                                      # b(x, y) = a(x - 3 k, y + 2 k)
        cases.append((a, b, bounds_for(k, 1.0, w // 2 - 2 * k, h // 2 + 2 * k), 1.0, S, 32))
    return cases


def expected(case):
    a, b, (x0, x1, y0, y1), scale, S, gain = case
    g = R.grid_of_bounds(x0, x1, y0, y1, scale)
    chip = R.block_means(a, g[1], g[2], g[0], R.C)
    return g, chip, R.search(chip, g, b, S, gain)


def test_host_build_of_the_motion_code_under_sanitizers(tmp_path):
    exe = B.host_program("track_motion_host", tmp_path)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for n, (a, b, bounds, scale, S, gain) in enumerate(cases):
        for img in (a, b):
            h, w = img.shape
            stride = (w | 1) + 2 * (n % 3)                                                 # an odd pitch
            buf = pitched(img, stride)
            blob.append(struct.pack("<4i", w, h, stride, buf.size) + buf.tobytes())
        blob.append(struct.pack("<5f2i", *bounds, scale, S, gain))
    triples = []
    for g in range(256):                                                                   # every min_gain boundary
        zero = 256 * 3 + 256 * (g % 5)
        best = zero // 256 * (256 - g)
        triples += [(best, zero, g), (best + 1, zero, g)]
    triples += [(0, 0, 255), (1, 0, 0), (261120, 261120, 0), (261120, 261120, 1)]
    blob.append(struct.pack("<i", len(triples)) + np.asarray(triples, np.int32).tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 300, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint8)
    at, ks, outside, moved = 0, set(), 0, 0

    def ints(n):
        nonlocal at
        v = got[at:at + 4 * n].view(np.int32)
        at += 4 * n
        return v

    for n, case in enumerate(cases):
        g, chip, s = expected(case)
        S = case[4]
        assert tuple(ints(3)) == g, n
        assert np.array_equal(got[at:at + 1024].reshape(32, 32), chip), n
        at += 1024
        assert np.array_equal(ints((2 * S + 1) ** 2).reshape(2 * S + 1, 2 * S + 1), s["table"]), n
        assert tuple(ints(6)) == (s["dx"], s["dy"], s["best"], s["zero"], s["shift"][0], s["shift"][1]), n
        ks.add(g[0])
        outside += int(not chip.any())
        moved += int(s["shift"] != (0, 0))
    want = [int(R.accept(*t)) for t in triples]
    assert ints(len(triples)).tolist() == want
    assert want[:512] == [1, 0] * 256                                                      # equality accepts, one more refuses
    assert at == got.size
    assert {1, 2, 5, 64} <= ks and outside >= 8 and moved >= 2
    print(f"{len(cases)} cases, cell sizes {sorted(ks)}, {outside} chips wholly outside, {moved} accepted shifts")


def test_properties_of_the_restatement():
    cases = host_cases()
    # a constant image: all SADs equal, the key picks (0, 0)
    for case in cases[-4:-2]:
        _, _, s = expected(case)
        assert (s["table"] == s["table"][0, 0]).all() and (s["dx"], s["dy"]) == (0, 0) and s["shift"] == (0, 0)
    # exact translations: SAD 0 at (3, -2), the shift (3 k, -2 k)
    for case, k in zip(cases[-2:], (1, 2)):
        g, _, s = expected(case)
        assert g[0] == k and (s["dx"], s["dy"], s["best"]) == (3, -2, 0) and s["shift"] == (3 * k, -2 * k)
    # the clamp of the centre, the cap of k, k = 1 for a face without size or a NaN
    assert R.grid_of_bounds(3.0e6, 3.0e6 + 8, -4.0e6, -4.0e6 + 8, 1.0) == (1, 2 ** 20 - 16, -2 ** 20 - 16)
    assert R.grid_of_bounds(0, 1e30, 0, 1, 4.0)[0] == 64 and R.grid_of_bounds(5, 5, 7, 7, 1.25) == (1, -11, -9)
    assert R.grid_of_bounds(np.nan, 1, 0, 1, 1.0)[0] == 1
    assert R.grid_of_bounds(0, 32, 0, 8, 1.0)[0] == 1 and R.grid_of_bounds(0, 32.5, 0, 8, 1.0)[0] == 2
    # ties go to the offset nearest (0, 0), then the smaller dy, then the smaller dx
    chip = np.zeros((32, 32), np.uint8)
    s = R.search(chip, (1, 0, 0), np.zeros((40, 40), np.uint8), 2, 0)
    assert (s["dx"], s["dy"]) == (0, 0)
    # the largest sums stay below 2^31
    assert 255 * 64 * 64 + 64 * 64 // 2 < 2 ** 31 and 255 * 1024 * 256 < 2 ** 31
    # the shift keeps a row's bits at (0, 0), -0.0 included
    row = np.array([[-0.0, 1.5, 2.0, 3.0]], f32)
    assert np.array_equal(R.shifted(row, [[0, 0]]).view(np.uint32), row.view(np.uint32))
    assert R.shifted(row, [[8, -4]]).tolist() == [[8.0, 9.5, -2.0, -1.0]]


def test_state_rules_of_the_restatement():
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (80, 96), dtype=np.uint8) for _ in range(2)]
    rows = np.stack([np.concatenate([rng.uniform(20, 70, 5), rng.uniform(15, 60, 5)]).astype(f32) for _ in range(2)])
    m = R.Motion(3, search=4, scale=1.25, min_gain=0)
    assert not m.search_step([0, 1], [True, True], imgs).any() and not m.last.any()       # nothing stored yet: not searched
    m.store_step([0, 1], rows, [0, 4], imgs)
    assert m.valid.tolist() == [True, False, False]                                        # a lost row stores nothing
    sh = m.search_step([1, 0], [True, True], imgs, idx=[1, 0])
    assert m.last[0, 5] == 1 and m.last[1, 5] == 0 and not sh[0].any()
    assert m.last[0, 2] == 0 and not sh[1].any()                                           # the same image: SAD 0 in place
    assert not m.search_step([0], [False], imgs).any() and m.last[0, 5] == 0               # a STARTED row is not searched
    m.invalidate([0])
    assert not m.get([0])[1].any() and not m.get([0])[2].any()


def test_symbols_and_python_arguments():
    assert {"sdm_track_configure_motion", "sdm_track_get_motion"} <= set(_lib.EXPORTED)
    text = open(os.path.join(B.ROOT, "include", "sdm.h")).read()
    assert "Tracking, motion-compensated" in text
    for word in ("sub-chip-pixel refinement", "rotation or scale search", "lost rule built on the SAD values"):
        assert word in text, word
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    modes = dict(re.findall(r"\b(SDM_TRACK_MOTION_\w+) = (\d+)", header))
    assert modes == {"SDM_TRACK_MOTION_OFF": "0", "SDM_TRACK_MOTION_SAD": "1"}
    for k, v in modes.items():
        assert getattr(_lib, k) == int(v), k
    assert re.search(r"\bsdm_track_configure_motion\s*\(\s*sdm_ctx\*\s*\w+,\s*int mode,\s*int search,\s*float scale,\s*int min_gain\)", header)
    assert re.search(r"\bsdm_track_get_motion\s*\(", header)
    assert Tracker._motion(None) is None and Tracker._motion(False) is None
    assert Tracker._motion(True) == (8, 1.25, 64) and Tracker._motion([16, 0.5, 0]) == (16, 0.5, 0)
    for bad in ((8, 1.25), 8, (0, 1.25, 32), (17, 1.25, 32), (8, 0.4, 32), (8, 4.5, 32), (8, np.nan, 32), (8, 1.25, -1), (8, 1.25, 256),
                (8.5, 1.25, 32), ("a", 1.25, 32)):
        with pytest.raises(ValueError):
            Tracker(None, 4, motion=bad)                            # (refused before the model or a device is looked at)
    tr = Tracker.__new__(Tracker)
    tr.motion_params = None
    with pytest.raises(ValueError):
        tr.motion([0])


def test_make_tracks_keywords_keep_todays_bytes():
    sig = inspect.signature(synth.make_tracks)
    assert sig.parameters["max_step"].default == 3.0 and sig.parameters["max_scale"].default == 0.03
    plain = synth.make_tracks(3, 4, seed=77, size=256)
    named = synth.make_tracks(3, 4, seed=77, size=256, max_step=3.0, max_scale=0.03)
    for a, b in zip(plain, named):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # the bytes of this call before the keywords existed
    assert hashlib.sha256(b"".join(a.tobytes() for a in plain)).hexdigest() == MAKE_TRACKS_SHA256
    fast = synth.make_tracks(3, 4, seed=77, size=256, max_step=20.0)
    steps = np.abs(np.diff(fast[2][:, :, :2].astype(int), axis=0))
    assert steps.max() > 3 and steps.max() <= 20
    assert np.array_equal(fast[2][0], synth.make_tracks(3, 4, seed=77, size=256)[2][0])    # the draws stay in their order


MAKE_TRACKS_SHA256 = "b737d1a4b81f235b5006a5e75a29328e85633aa2501a85a29d5c924297806e59"
