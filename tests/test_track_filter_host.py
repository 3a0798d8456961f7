"""The tracker's temporal landmark filter without a device: what the One-Euro filter of include/sdm.h ("Tracking, filtered") does to
noise and to motion, on its numpy restatement (tests/track_filter_ref.py); its state rules; the kernel's per-row and per-coordinate
code compiled for the host (tests/cpp/track_filter_host.cpp, address and undefined-behaviour sanitizers, every state row in a heap
block of exactly 2L floats) against the restatement, bit for bit; the exported symbols and the Python argument handling."""
import os
import re
import struct

import numpy as np
import pytest

import cpp_build as B
import landmark_count_cases as K
import track_filter_ref as F
from superviseddescent_amd import _lib, ibug
from superviseddescent_amd.engine import Tracker

f32 = np.float32
DT = f32(1.0 / 30.0)
COUNTS = [2, 22, 32, 33, 72]            # the landmark counts of the device parity test (tests/test_gpu_track_filter.py)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def face(L, size=100.0, origin=(80.0, 60.0)):
    """a row of L landmarks about `size` pixels wide"""
    m = K.mean(L) if L != 22 else ibug.select_mean(ibug.RCR22_IDS)
    x = np.concatenate([(m[:L] + f32(0.5)) * f32(size) + f32(origin[0]), (m[L:] + f32(0.5)) * f32(size) + f32(origin[1])])
    return x.astype(f32)


@pytest.mark.parametrize("min_cutoff", [0.5, 1.0, 3.0])
def test_white_noise_is_attenuated_as_a_first_order_low_pass(min_cutoff):
    """beta = 0: a stationary row with N(0, 0.5 px) noise, 4 000 frames at 30 Hz, the first 200 dropped.  The output's standard
    deviation over the input's is sqrt(alpha / (2 - alpha)) for white noise through y += alpha (x - y): within 5 %."""
    L, n = 22, 4000
    base = face(L)
    noise = np.random.default_rng(20260).normal(0.0, 0.5, (n, 2 * L)).astype(f32)
    flt = F.OneEuro(1, L, min_cutoff, 0.0, 1.0)
    x = base[None, :] + noise
    out = np.stack([flt.step([0], x[t], 0, DT)[0] for t in range(n)])
    assert np.array_equal(bits(out[0]), bits(x[0]))
    sd_in = np.sqrt(np.mean(np.var(x[200:].astype(np.float64), axis=0)))
    sd_out = np.sqrt(np.mean(np.var(out[200:].astype(np.float64), axis=0)))
    a = F.alpha_exact(min_cutoff, 1.0 / 30.0)
    want = np.sqrt(a / (2.0 - a))
    print(f"min_cutoff {min_cutoff}: sd out / sd in {sd_out / sd_in:.4f}, derived {want:.4f}")
    assert abs(sd_out / sd_in - want) <= 0.05 * want
    assert flt.guards == [0, 0]


def steady_lag(beta, n=400):
    """the row moves at 60 px/s in x (2 px per frame: every position is exact in float32); the lag of the last frame"""
    L = 22
    base = face(L)
    flt = F.OneEuro(1, L, 1.0, beta, 1.0)
    lags = []
    for t in range(n):
        x = base.copy()
        x[:L] += f32(2 * t)
        out = flt.step([0], x, 0, DT)[0]
        lags.append((x[:L].astype(np.float64) - out[:L]).mean())
        assert np.abs(out[L:] - x[L:]).max() <= 1e-4               # (what does not move stays: roundings of 1.5e-5 at 170, summed over 1 / alpha steps)
    assert abs(lags[-1] - lags[-2]) < 1e-4                          # steady
    return lags[-1]


def test_constant_velocity_lag_falls_with_beta():
    a = F.alpha_exact(1.0, 1.0 / 30.0)
    want = 60.0 * (1.0 / 30.0) * (1.0 - a) / a
    lag0, lag5, lag20 = steady_lag(0.0), steady_lag(5.0), steady_lag(20.0)
    print(f"steady lag at 60 px/s, face 100 px, min_cutoff 1: beta 0 {lag0:.4f} (derived {want:.4f}), beta 5 {lag5:.4f}, beta 20 {lag20:.4f}")
    assert abs(want - 9.549) < 1e-3 and abs(lag0 - want) <= 1e-3
    assert 0 < lag20 < lag5 < lag0


def test_state_rules():
    L = 22
    rng = np.random.default_rng(3)
    rows = [face(L) + rng.normal(0, 0.5, 2 * L).astype(f32) for _ in range(6)]
    flt = F.OneEuro(3, L, 1.0, 5.0)
    assert not flt.get([0, 1, 2])[2].any() and not flt.get([1])[0].any()
    out = flt.step([1], rows[0], 0, DT)
    assert np.array_equal(bits(out[0]), bits(rows[0]))                         # the first step returns x's bits
    fr, d, primed = flt.get([0, 1, 2])
    assert primed.tolist() == [0, 1, 0] and np.array_equal(bits(fr[1]), bits(rows[0])) and not d.any() and not fr[[0, 2]].any()
    out = flt.step([1], rows[1], 0, DT)
    assert not np.array_equal(bits(out[0]), bits(rows[1]))                     # the second is filtered
    assert (np.abs(out[0] - rows[0]) <= np.abs(rows[1] - rows[0]) + 1e-4).all()
    out = flt.step([1], rows[2], 4, DT)                                        # a lost row returns x and un-primes
    assert np.array_equal(bits(out[0]), bits(rows[2])) and flt.get([1])[2][0] == 0 and not flt.get([1])[0].any()
    out = flt.step([1], rows[3], 0, DT)                                        # the row after it re-primes
    assert np.array_equal(bits(out[0]), bits(rows[3])) and flt.get([1])[2][0] == 1
    flt.unprime([1])                                                           # a restart
    out = flt.step([1], rows[4], 0, DT)
    assert np.array_equal(bits(out[0]), bits(rows[4]))
    assert flt.get([0, 2])[2].tolist() == [0, 0]                               # the other slots were never touched
    # a face without size: no speed weight, the filter is min_cutoff's low-pass
    point = np.full(2 * L, 7.0, f32)
    a, b = F.OneEuro(1, L, 1.0, 5.0), F.OneEuro(1, L, 1.0, 0.0)
    for t in range(3):
        ra, rb = a.step([0], point + f32(t), 0, DT), b.step([0], point + f32(t), 0, DT)
        assert np.array_equal(bits(ra), bits(rb))


def host_cases():
    """per landmark count two parameter sets; 5 slots, 16 ops: random subsets of the ids in random order, lost rows, a restart, dt
    drawn over [1e-4, 1e4] and at either bound; rows of a moving face, then the special ones -- a face without size (s = 0),
    coordinates of +-3e38 against a state of the other sign (the derivative is not finite), and a face of 1.2e-38 pixels seen twice
    (beta / s is infinite, times a derivative of 0: the filtered value is not finite)"""
    cases = []
    for L in COUNTS:
        for params in ((1.0, 5.0, 1.0), (0.5, 20.0, 2.5)):
            rng = np.random.default_rng(100 * L + int(params[1]))
            S, M = 5, 2 * L
            pos = np.stack([face(L, 60.0 + 40.0 * s, (30.0 * s, 20.0 * s)) for s in range(S)])
            ops = []
            for o in range(16):
                if o == 9:
                    ops.append(("unprime", np.array([1, 3], np.int32)))
                    continue
                ids = rng.permutation(S)[:rng.integers(1, S + 1)].astype(np.int32)
                if o in (4, 5, 6, 7, 8, 12, 13, 14):               # the special rows are slot 0's, first in the step
                    ids = np.concatenate([[0], ids[ids != 0]]).astype(np.int32)
                pos[ids] += rng.normal(0, 1.5, (ids.size, M)).astype(f32) + f32(2.0)
                x = pos[ids].copy()
                masks = (rng.random(ids.size) < 0.15).astype(np.int32) * rng.integers(1, 16, ids.size).astype(np.int32)
                dt = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), ids.size)).astype(f32)
                dt[0] = (f32(1e-4), f32(1e4), DT)[o % 3]
                if o in (4, 5):
                    x[0] = f32(12.5) + f32(o)                      # s = 0, twice
                    masks[0] = 0
                if o in (6, 7, 8):
                    x[0] = f32(3e38) * f32((-1) ** o)              # +-3e38: x - r overflows
                    x[0, ::3] = f32(-3e38) * f32((-1) ** o)
                    masks[0] = 0
                if o in (12, 13, 14):
                    x[0] = 0                                       # a face of 1.2e-38 pixels that does not move: lost, primed
                    x[0, L - 1] = f32(1.2e-38)                     # (d = 0), then filtered with v = 0
                    masks[0] = 2 if o == 12 else 0
                ops.append(("step", ids, masks, dt, x))
            cases.append((L, S, params, ops))
    return cases


def test_host_build_of_the_filter_code_under_sanitizers(tmp_path):
    exe = B.host_program("track_filter_host", tmp_path)
    cases = host_cases()
    blob = [struct.pack("<i", len(cases))]
    for L, S, params, ops in cases:
        blob.append(struct.pack("<3i3f", L, S, len(ops), *params))
        for op in ops:
            if op[0] == "unprime":
                blob.append(struct.pack("<2i", 1, op[1].size) + op[1].tobytes())
            else:
                _, ids, masks, dt, x = op
                blob.append(struct.pack("<2i", 0, ids.size) + ids.tobytes() + masks.tobytes() + dt.tobytes() + x.tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    B.run(exe, [tmp_path / "cases.bin", tmp_path / "out.bin"], 120, sanitized=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.uint32)
    at, guards, lost, filtered = 0, np.zeros(2, int), 0, 0
    for L, S, params, ops in cases:
        M = 2 * L
        flt = F.OneEuro(S, L, *params)
        for o, op in enumerate(ops):
            if op[0] == "unprime":
                flt.unprime(op[1])
                continue
            _, ids, masks, dt, x = op
            filtered += int(((masks == 0) & (flt.primed[ids] != 0)).sum())
            want = flt.step(ids, x, masks, dt)
            assert np.array_equal(got[at:at + ids.size * M].reshape(-1, M), bits(want)), (L, params, o)
            at += ids.size * M
            lost += int((masks != 0).sum())
        for state in (flt.r, flt.d, flt.f):
            assert np.array_equal(got[at:at + S * M].reshape(S, M), bits(state)), (L, params)
            at += S * M
        assert np.array_equal(got[at:at + S].view(np.int32), flt.primed)
        at += S
        assert flt.guards[0] > 0 and flt.guards[1] > 0, (L, params, flt.guards)      # both non-finite guards were taken
        guards += flt.guards
    assert at == got.size
    print(f"{len(cases)} cases: {filtered} filtered rows, {lost} lost rows, non-finite derivative {guards[0]}, filtered value {guards[1]}")
    assert lost >= 10 and filtered >= 200


def test_symbols_and_python_arguments():
    assert {"sdm_track_configure_filter", "sdm_track_step_filtered", "sdm_track_get_filtered"} <= set(_lib.EXPORTED)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(B.ROOT, "include", "sdm.h")).read(), flags=re.S)
    modes = dict(re.findall(r"\b(SDM_TRACK_FILTER_\w+) = (\d+)", header))          # (an enum beside the step's prototypes)
    assert modes == {"SDM_TRACK_FILTER_OFF": "0", "SDM_TRACK_FILTER_ONE_EURO": "1"}
    for k, v in modes.items():
        assert getattr(_lib, k) == int(v), k
    for n in ("sdm_track_configure_filter", "sdm_track_step_filtered", "sdm_track_get_filtered"):
        assert re.search(r"\b%s\s*\(" % n, header), n
    assert Tracker._smooth(None) is None
    assert Tracker._smooth((1, 0.5)) == (1.0, 0.5, 1.0) and Tracker._smooth([0.5, 0, 2]) == (0.5, 0.0, 2.0)
    for bad in ((1.0,), (1.0, 2.0, 3.0, 4.0), 1.0, (0.0, 1.0), (1.0, -1.0), (1.0, 1.0, 0.0), (np.nan, 1.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            Tracker(None, 4, smooth=bad)                           # (refused before the model or a device is looked at)
    tr = Tracker.__new__(Tracker)
    tr.smooth = None
    with pytest.raises(ValueError):
        tr.step([0, 1], dt=1 / 30)                                 # dt without smooth
    with pytest.raises(ValueError):
        tr.get_filtered([0])
    tr.smooth = (1.0, 5.0, 1.0)
    with pytest.raises(ValueError):
        tr.step([0, 1], dt=[1 / 30] * 3)                           # neither one value nor one per id
