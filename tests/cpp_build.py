"""How the tests build and run the C++ programs of tests/cpp, and what their scenarios share: the one command line of a device driver
(*_gpu.cpp on gpu_driver.hpp, against libsdm_hip.so), the one of a host program (*_host.cpp on host_case.hpp, the kernels' per-pixel
code under the address and undefined-behaviour sanitizers), the child-process run, the random-regressor model file, and the frame
lists of a placed buffer (align_tensor_cases.place).  A plain module, imported like paste_cases."""
import os
import subprocess

import numpy as np

import align_tensor_cases as K
import align_tensor_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "superviseddescent_amd", "lib")


def gpu_driver(name, out_dir, src=None, opt=("-O2",), link=True):
    """tests/cpp/<name>.cpp (or src) built against the headers and libsdm_hip.so into out_dir; the executable's path.  link False:
    compiled only, <name>.o"""
    out = os.path.join(str(out_dir), name if link else name + ".o")
    cmd = ["g++", "-std=c++17", *opt, "-Wall", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "superviseddescent_amd", "include")]
    src = str(src) if src else os.path.join(CPP, name + ".cpp")
    cmd += [src, "-o", out, "-L" + LIB, "-lsdm_hip", "-Wl,-rpath," + LIB, "-lpthread", "-ldl"] if link else ["-c", src, "-o", out]
    subprocess.check_call(cmd)
    return out


def host_program(name, out_dir):
    """tests/cpp/<name>.cpp -- device functions with their own main, no device -- built for the host under the sanitizers"""
    out = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(CPP, name + ".cpp"), "-o", out])
    return out


def run(exe, args, timeout, sanitized=False):
    """one child process: its stdout printed, status 0 asserted; sanitized: a host_program, with the sanitizers' options"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1") if sanitized else None
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def write_model(d, L, params, mean, ids, seed=4321, regressors=None):
    """<d>/model.bin: a detection model of one regressor per level of params -- the given matrices, or random ones drawn from seed (a
    Generator passes through: a test that goes on drawing hands in its own).  Returns the matrices."""
    from superviseddescent_amd import ibug, model_io
    if regressors is None:
        rng = np.random.default_rng(seed)
        regressors = [rng.normal(0, 3e-3, (L * p.patch_dim + 1, 2 * L)).astype(np.float32) for p in params]
    model_io.save_detection_model(model_io.DetectionModelFile(
        [model_io.RegressorRecord(r, 1, 1.5, False) for r in regressors], mean, ids,
        [(p.vlhog_variant, p.num_cells, p.cell_size, p.num_bins, p.relative_patch_size) for p in params],
        ibug.RIGHT_EYE_IDS, ibug.LEFT_EYE_IDS), os.path.join(str(d), "model.bin"))
    return regressors


def device_frames(dev, frames):
    """the frames of a placed buffer that is on the device (a torch tensor) as the Python layer's frame list"""
    return [(dev.data_ptr() + fr["off"], fr["w"], fr["h"], fr["stride"], K.NAMES[fr["fmt"]]) for fr in frames]


def device_chroma(dev, frames, only_separate=False):
    """their UV planes: a pointer per NV12 frame (only_separate: per NV12 frame whose UV plane is placed apart), None otherwise"""
    return [dev.data_ptr() + fr["uv_off"] if fr["fmt"] == T.NV12 and (not only_separate or fr["separate"]) else None for fr in frames]
