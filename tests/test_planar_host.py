"""Planar colour frames without a device: the shared device headers' planar paths -- the crop tensors' pixel fetch, the area sums of the
rigid crop and of the warp, the pastes' load / apply / store -- compiled for the host (tests/cpp/planar_host.cpp, address and
undefined-behaviour sanitizers, every frame in a heap block of exactly the bytes it owns) and compared inside the program with the same
functions on the interleaved frame of the same pixels: planes at the default, a padded odd and a negative distance, faces over all four
borders, frames 2 pixels wide and 1 x 1."""
import cpp_build as B


def test_planar_fetch_and_paste_match_the_interleaved_frame(tmp_path):
    out = B.run(B.host_program("planar_host", tmp_path), [], timeout=300, sanitized=True)
    assert "24 cases" in out.stdout
