"""rcr::DeviceFrame's second plane in the C++ header layer (superviseddescent_amd/include/rcr/adaptive_vlhog.hpp, alignment.hpp;
tests/cpp/planar_gpu.cpp): planar BGR frames -- planes a padded distance apart through `second_plane`, and contiguous 3 x H x W blocks
through the aggregate form of old -- give, through detect_batch, one crop tensor and one paste, the bytes of the interleaved frames of
the same pixels; the bytes between the planes stay what they were."""
import os

import numpy as np
import pytest

import cpp_build as B
import paste_cases as C


@pytest.mark.gpu
def test_cpp_planar_frames_match_the_interleaved_frames(built, tmp_path):
    from superviseddescent_amd import HoGParam, ibug, synth
    from test_gpu_align_tensor import LM, template
    ids = ibug.RCR22_IDS
    L = len(ids)
    params = [HoGParam(1, 5, 6, 4, 0.6), HoGParam(1, 5, 4, 4, 0.4)]
    d = str(tmp_path)
    rng = np.random.default_rng(4321)
    B.write_model(d, L, params, ibug.select_mean(ids), ids, seed=rng)
    tracks, _, boxes = synth.make_tracks(3, 1, seed=57)                        # frames x streams x H x W
    cut = ((slice(0, 230), slice(0, 256)), (slice(0, 256), slice(0, 241)), (slice(0, 199), slice(0, 233)))      # three sizes
    S, w, h = 3, 16, 16
    colour = []
    for s in range(S):
        g = tracks[0, s][cut[s]]
        c = rng.integers(0, 256, g.shape + (3,), dtype=np.uint8)
        c[..., 1] = g
        colour.append(c)
    with open(os.path.join(d, "frames.u8"), "wb") as f:
        for c in colour:
            f.write(c.tobytes())
    boxes[0].astype(np.int32).tofile(os.path.join(d, "boxes.i32"))
    template(w, h).tofile(os.path.join(d, "tmpl.f32"))
    C.tensor(S, w, h, "float16", "nchw", 3, 19).tofile(os.path.join(d, "tensor.f16"))
    C.alpha_maps(S, w, h, 20).tofile(os.path.join(d, "alpha.u8"))
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{S} {w} {h} {len(LM)} " + " ".join(map(str, LM)) + "\n")
        f.write("".join(f"1 {c.shape[1]} {c.shape[0]} {3 * c.shape[1]} {c.size}\n" for c in colour))
    B.run(B.gpu_driver("planar_gpu", tmp_path), [d], 300)
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    rows = rd("rows_packed.f32", np.float32)
    assert rows.size == S * 2 * L and np.isfinite(rows).all()
    for name in ("rows_%s.f32", "crops_%s.u8", "mats_%s.f32", "flags_%s.i32"):
        assert rd(name % "planar", np.uint8).tobytes() == rd(name % "packed", np.uint8).tobytes(), name
    assert rd("crops_packed.u8", np.uint8).any()
    packed, planar = rd("paste_packed.u8", np.uint8), rd("paste_planar.u8", np.uint8)
    assert not np.array_equal(packed, np.concatenate([c.reshape(-1) for c in colour]))          # the paste wrote
    at_k, at_p = 0, 0
    for s, c in enumerate(colour):
        H, W = c.shape[:2]
        D = H * W + (67 if s % 2 == 0 else 0)
        want = packed[at_k:at_k + c.size].reshape(H, W, 3)
        block = planar[at_p:at_p + 2 * D + H * W]
        for k in range(3):
            assert np.array_equal(block[k * D:k * D + H * W].reshape(H, W), want[..., k]), (s, k)
            assert (block[k * D + H * W:(k + 1) * D] == 0xA5).all()                              # the bytes between the planes
        at_k += c.size
        at_p += 2 * D + H * W
    assert at_p == planar.size
