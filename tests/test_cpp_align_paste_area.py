"""The rcr::paste_crops_tensor overloads that take an rcr::AlignFilter (superviseddescent_amd/include/rcr/alignment.hpp,
tests/cpp/align_paste_area_gpu.cpp): landmark rows on gray, BGR, RGBA and BGRA DeviceFrames, the crop larger than the face, give in both
forms the bytes and the S of the Python layer on the same rows, tensor, opacity maps and frames -- the same kernels behind the same
C-ABI --, and those are the restatement's."""
import os

import numpy as np
import pytest

import align_tensor_cases as K
import cpp_build as B
import paste_area_cases as D
import paste_area_ref as Q
import paste_cases as C


@pytest.mark.gpu
def test_cpp_filtered_paste_matches_python(built, tmp_path):
    import torch
    from superviseddescent_amd import Context, HoGParam, ibug
    from test_gpu_align_tensor import IDS as ids, L, LM, MEAN as mean, template
    params = [HoGParam(1, 5, 6, 4, 0.6)]
    buf, frames = C.place([C.FRAMES[0], C.FRAMES[1], C.FRAMES[6], C.FRAMES[4]], 17)
    w, h, S = 16, 16, 4
    tmpl = template(w, h)
    sims = [D.minifying(frames[r], w, h, 18 + r, 1, D.W_SCALES[r + 1:] + D.W_SCALES[:r + 1])[0] for r in range(S)]     # W scales 1.7, 2.6, 4.5, 20
    x = K.landmark_rows(sims, tmpl, LM, L)
    y = C.tensor(S, w, h, "float16", "nchw", 3, 19)
    alpha = C.alpha_maps(S, w, h, 20, zero_band=True)
    d = str(tmp_path)
    B.write_model(d, L, params, mean, ids)
    meta = [f"{S} {w} {h} {len(LM)} " + " ".join(map(str, LM)) + "\n"]
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for fr in frames:
            f.write(buf[fr["off"]:fr["off"] + fr["h"] * fr["stride"]].tobytes())
            meta.append(f"{fr['fmt']} {fr['w']} {fr['h']} {fr['stride']} {fr['h'] * fr['stride']}\n")
    x.tofile(os.path.join(d, "rows.f32"))
    tmpl.tofile(os.path.join(d, "tmpl.f32"))
    y.tofile(os.path.join(d, "tensor.f16"))
    alpha.tofile(os.path.join(d, "alpha.u8"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write("".join(meta))
    B.run(B.gpu_driver("align_paste_area_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    c = Context(0)
    try:
        re_, le_ = ibug.eye_indices(ids)
        c.set_model_geometry(L, re_, le_, params)
        dev = torch.from_numpy(buf).cuda()
        lst = B.device_frames(dev, frames)
        c.set_frames_device(lst)
        c.set_sample_image_index(None)
        c.set_x(x)
        spec = dict(scale=C.SCALES, bias=C.BIASES)
        mats, flags, samples = c.align_paste_tensor(LM, tmpl, torch.from_numpy(y).cuda(), lst, mask=alpha, filter="area", **spec)
        got = dev.cpu().numpy()
        assert rd("mats.f32", np.uint32).tobytes() == mats.tobytes()
        assert np.array_equal(rd("flags.i32", np.int32), flags) and np.array_equal(rd("flags_at.i32", np.int32), flags)
        assert np.array_equal(rd("samples.i32", np.int32), samples) and np.array_equal(rd("samples_at.i32", np.int32), samples)
        assert samples.tolist() == [Q.samples(m) for m in mats] and len(set(samples.tolist())) >= 3 and samples.min() > 1
        mine = np.concatenate([got[fr["off"]:fr["off"] + fr["h"] * fr["stride"]] for fr in frames])
        assert np.array_equal(rd("fit.u8", np.uint8), mine) and np.array_equal(rd("at.u8", np.uint8), mine)
        want = buf.copy()
        for r, fr in enumerate(frames):
            Q.paste_row(C.view(want, fr), fr["fmt"], mats[r], y[r], alpha[r], int(samples[r]), **spec)
        assert np.array_equal(got, want) and (want != buf).sum() > 100
    finally:
        c.close()
