"""The rcr::paste_warped_tensor overloads that take the frames' UV planes (superviseddescent_amd/include/rcr/warp.hpp,
tests/cpp/warp_paste_nv12_gpu.cpp): landmark rows on NV12 DeviceFrames -- the UV plane behind Y or in an allocation of its own -- and a
BGR one give, through the fit and through explicit points, the bytes of the restatement (tests/warp_paste_nv12_ref.py); an empty chroma
vector means every UV plane lies behind its Y plane."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import align_tensor_ref as T
import cpp_build as B
import paste_cases as C
import paste_nv12_cases as V
import warp_paste_nv12_ref as WN
import warp_paste_ref as WP
import warp_ref as R


def test_cpp_driver_compiles(tmp_path):
    """the new overloads and their driver build against the headers without a device"""
    B.gpu_driver("warp_paste_nv12_gpu", tmp_path, link=False)


@pytest.mark.gpu
def test_cpp_nv12_warp_paste_matches_the_restatement(built, tmp_path):
    from superviseddescent_amd import HoGParam, alignment_template, delaunay
    from test_gpu_align_tensor import IDS as ids, L, MEAN as mean
    LM = np.arange(L)                                          # the RCR-22 mesh: every landmark
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = V.place([V.FRAMES[0], V.FRAMES[1], V.FRAMES[7], V.FRAMES[6]], 17)
    w, h, S = 24, 20, 4
    tmpl = alignment_template(mean, LM, w, h, 0.1)
    tri = delaunay(tmpl)
    lab = R.labels(tmpl, tri, w, h)
    x = K.landmark_rows(K.similarities(frames, range(S), w, h, 18), tmpl, LM, L)
    y = C.tensor(S, w, h, "float16", "nchw", 3, 19)
    alpha = C.alpha_maps(S, w, h, 20, zero_band=True)
    d = str(tmp_path)
    B.write_model(d, L, params, mean, ids)
    meta = [f"{S} {w} {h} {len(LM)} " + " ".join(map(str, LM)) + "\n"]

    def planes_of(b):
        """the frames' bytes as the driver lays them out: plane 0 (h rows of the pitch), then the UV plane"""
        out = []
        for fr in frames:
            out.append(b[fr["off"]:fr["off"] + fr["h"] * fr["stride"]])
            if fr["fmt"] == T.NV12:
                out.append(b[fr["uv_off"]:fr["uv_off"] + (fr["h"] + 1) // 2 * fr["stride"]])
        return np.concatenate(out)

    full = np.concatenate([buf, np.zeros(256, np.uint8)])                        # (whole pitches of the last plane lie inside)
    planes_of(full).tofile(os.path.join(d, "frames.u8"))
    for fr in frames:
        nv = fr["fmt"] == T.NV12
        meta.append(f"{fr['fmt']} {fr['w']} {fr['h']} {fr['stride']} {fr['h'] * fr['stride']} "
                    f"{(fr['h'] + 1) // 2 * fr['stride'] if nv else 0} {int(nv and fr['separate'])}\n")
    x.tofile(os.path.join(d, "rows.f32"))
    tmpl.tofile(os.path.join(d, "tmpl.f32"))
    y.tofile(os.path.join(d, "tensor.f16"))
    alpha.tofile(os.path.join(d, "alpha.u8"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("".join(meta))
    B.run(B.gpu_driver("warp_paste_nv12_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    pts = WP.points_of(x, LM)
    mats = WP.matrices(pts, tmpl, tri)
    assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes()
    flags = WP.flags(pts, tmpl, tri, [(fr["w"], fr["h"]) for fr in frames])
    assert np.array_equal(rd("flags.i32", np.int32), flags) and np.array_equal(rd("flags_at.i32", np.int32), flags)
    spec = dict(scale=C.SCALES, bias=C.BIASES)
    want = full.copy()
    for r, fr in enumerate(frames):
        if fr["fmt"] == T.NV12:
            WN.paste_row(*V.planes(want, fr), pts[r], tri, mats[r], lab, y[r], alpha[r], **spec)
        else:
            WP.paste_row(C.view(want, fr), fr["fmt"], pts[r], tri, mats[r], lab, y[r], alpha[r], **spec)
    assert (want != full).sum() > 500
    assert np.array_equal(rd("fit.u8", np.uint8), planes_of(want)) and np.array_equal(rd("at.u8", np.uint8), planes_of(want))
    # the empty chroma vector: every UV plane behind its Y plane -- the driver laid the planes out so; the same bytes plane by plane
    assert np.array_equal(rd("behind.u8", np.uint8), planes_of(want))
