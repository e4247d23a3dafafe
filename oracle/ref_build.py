#!/usr/bin/env python3
"""Builds oracle/_ref/ -- the part of the REFERENCE that compiles here from its own sources, where they lie (TEST INFRASTRUCTURE).

Two builds:

1. `build()` (CPU, runs anywhere): `palette/src/bindings.cpp` (plain C++ / pybind11; holds compute_RGB_histogram, bindings.cpp:40-91), compiled
   UNMODIFIED from /root/reference with g++ against the torch / pybind11 headers of this image.  The two symbols it takes from palette.cu
   (rgb_to_hsv / hsv_to_rgb, palette/src/palette_func.h) come from this repo's PRODUCT binding of the C ABI for that extension
   (palettenerf_amd/csrc/shim/palette_func_hip.cpp -> libpnr_hip.so): reference pybind layer + reference histogram code + this repo's kernels.
2. `build_hip()` (round 4): the reference's CUDA extensions themselves -- raymarching/src/{raymarching.cu,bindings.cpp},
   shencoder/src/{shencoder.cu,bindings.cpp}, palette/src/{palette.cu,bindings.cpp} -- compiled UNMODIFIED for gfx950 with
   torch.utils.cpp_extension (torch's own hipify pass + hipcc; no header, library or tool is stood in for).  The sources are read where they lie;
   hipify writes its translated copies into a scratch directory under /tmp; only the resulting ref_<name>.so files are copied into oracle/_ref/.
   gridencoder/src/{gridencoder.cu,bindings.cpp} is built the same way; where its one call of atomicAdd(__half2*, __half2) has no overload in the
   HIP headers, a second attempt forces oracle/ref_half2_atomic.h (that overload alone, this repository's) in front of the unmodified source.
   tests/test_gpu_reference_kernels.py, tests/test_gpu_reference_grid.py and profiles/reference_kernels.py run these modules on the MI355X next to
   this repository's kernels.

Use: tests/golden/gen_golden.py imports the module to write tests/golden/hist.npz; tests/test_oracle.py checks the oracle's
compute_RGB_histogram against the module directly when it is present.  Outputs only into oracle/_ref/ (git-ignored, travels to the GPU box).
Nothing here runs on the GPU box: /root/reference does not exist there; the prebuilt .so is used as it is.
"""
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
REF_SRC = "/root/reference/palette/src/bindings.cpp"
SHIM = os.path.join(ROOT, "palettenerf_amd", "csrc", "shim", "palette_func_hip.cpp")
OUT_DIR = os.path.join(HERE, "_ref")
OUT = os.path.join(OUT_DIR, "_palette_func" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


def available():
    return os.path.exists(OUT)


def build(force=False, verbose=False):
    """Compile if /root/reference is present and the output is stale; returns the module path or None (no reference here, nothing prebuilt)."""
    if not os.path.exists(REF_SRC):
        return OUT if available() else None
    lib = os.path.join(ROOT, "palettenerf_amd", "libpnr_hip.so")
    deps = [REF_SRC, SHIM, os.path.join(ROOT, "include", "pnr.h")]
    if not force and available() and os.path.getmtime(OUT) >= max(os.path.getmtime(d) for d in deps):
        return OUT
    if not os.path.exists(lib):
        raise RuntimeError("build libpnr_hip.so first (python -m palettenerf_amd.build): the reference's _palette_func links against it")
    import torch
    from torch.utils import cpp_extension as ce
    os.makedirs(OUT_DIR, exist_ok=True)
    inc = [f"-I{p}" for p in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}"]
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DTORCH_EXTENSION_NAME=_palette_func", "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", "-w", *inc, REF_SRC, SHIM, "-o", OUT,
           f"-L{tlib}", "-ltorch", "-ltorch_cpu", "-lc10", "-ltorch_python", f"-L{os.path.dirname(lib)}", "-l:libpnr_hip.so",
           f"-Wl,-rpath,{tlib}", "-Wl,-rpath,$ORIGIN/../../palettenerf_amd"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return OUT


# ------------------------------------------------------------------------------------------------------------------------------------------
# Round 4: the reference's CUDA extensions themselves, compiled for gfx950 by the image's own toolchain for CUDA extensions on ROCm.
#
# torch.utils.cpp_extension (what the reference's */backend.py call) translates a .cu with torch.utils.hipify and compiles it with hipcc -- that is
# how ANY CUDA extension is built on a ROCm PyTorch, no file of this repository is involved.  The reference's own recipe fails here only because
# it passes -std=c++14 (raymarching/backend.py:7,12) to a torch 2.10 whose headers need C++17; with -std=c++17 (and the HIP spelling of its
# -U__CUDA_NO_HALF_* flags) three of the four extensions compile UNMODIFIED from /root/reference:
#     _raymarching (raymarching.cu: all 14 kernels), _shencoder (shencoder.cu), _palette_func (palette.cu + bindings.cpp).
# _gridencoder is tried the same way first.  Where that fails -- gridencoder.cu:303 calls atomicAdd(__half2*, __half2), an overload ROCm 7.2's
# headers do not have (they offer unsafeAtomicAdd) -- it is built a second time with oracle/ref_half2_atomic.h forced in front of the translation
# unit (-include): this repository's declaration of that ONE overload on unsafeAtomicAdd, nothing else.  The source text stays the reference's,
# unmodified.  What the stand-in covers is the table gradient of an fp16 table with an even feature count, the only caller of that overload: there
# the accumulation primitive is this repository's.  kernel_grid (forward, dy_dx), kernel_input_backward and the whole fp32 path are the reference's
# own code on the reference's own calls.  Which of the two builds produced the file is returned (key "gridencoder_build"), printed, and kept next to
# the file (oracle/_ref/ref_gridencoder.build.txt) for the GPU box.
# hipify writes its translation next to the input, /root/reference is read-only: the sources are copied to a scratch directory OUTSIDE the
# repository, built there, and only the .so files are kept (oracle/_ref/ref_<name>.so).  On the GPU box the tests load them and run the
# reference's own kernels on the MI355X next to this repository's (tests/test_gpu_reference_kernels.py, tests/test_gpu_reference_grid.py);
# bench.py times the first three (extra.reference_kernels).
HIP_EXTENSIONS = {
    "raymarching": ("_raymarching", ("raymarching.cu", "bindings.cpp")),
    "shencoder": ("_shencoder", ("shencoder.cu", "bindings.cpp")),
    "palette": ("_palette_func", ("palette.cu", "bindings.cpp")),
    "gridencoder": ("_gridencoder", ("gridencoder.cu", "bindings.cpp")),
}
STAND_IN = {"gridencoder": os.path.join(HERE, "ref_half2_atomic.h")}      # extensions with a second attempt: the header forced in front of the .cu
REF_ROOT = "/root/reference"


def hip_path(ext):
    return os.path.join(OUT_DIR, f"ref_{ext}.so")


def hip_available(ext):
    return os.path.exists(hip_path(ext))


def hip_build_note(ext):
    """How oracle/_ref/ref_<ext>.so was built ("unmodified", or "with <header>" after the unmodified attempt failed), and the seconds it took; None if unknown."""
    p = os.path.join(OUT_DIR, f"ref_{ext}.build.txt")
    return open(p).read().strip() if os.path.exists(p) else None


def _build_one(ext, modname, files, dst, verbose, include=None):
    import shutil
    import tempfile
    from torch.utils import cpp_extension as ce
    tmp = tempfile.mkdtemp(prefix="pnr_refbuild_", dir="/tmp")
    try:
        shutil.copytree(os.path.join(REF_ROOT, ext, "src"), os.path.join(tmp, "src"))      # scratch copy, outside the repository: hipify writes next to its input
        bd = os.path.join(tmp, "build")
        os.makedirs(bd)
        half = ["-U__CUDA_NO_HALF_OPERATORS__", "-U__CUDA_NO_HALF_CONVERSIONS__", "-U__CUDA_NO_HALF2_OPERATORS__"]       # the reference's own flags (backend.py:8) ...
        half += [f.replace("CUDA", "HIP") for f in half]                                                              # ... and their HIP spelling
        forced = ["-include", include] if include else []
        # a second build of one name in one process would be named <name>_v1 (PyInit symbol included): forget the first.  Should a later torch keep its
        # versions elsewhere, the copy below finds no <name>.so and says so
        entries = getattr(getattr(ce, "JIT_EXTENSION_VERSIONER", None), "entries", None)
        if isinstance(entries, dict):
            entries.pop(modname, None)
        ce.load(name=modname, extra_cflags=["-O3", "-std=c++17"], extra_cuda_cflags=["-O3", "-std=c++17", *half, *forced],
                sources=[os.path.join(tmp, "src", f) for f in files], build_directory=bd, verbose=verbose, is_python_module=False)
        built = os.path.join(bd, modname + ".so")
        if not os.path.exists(built):
            raise RuntimeError(f"{ext}: the build left no {modname}.so in its directory (found: {sorted(os.listdir(bd))})")
        os.makedirs(OUT_DIR, exist_ok=True)
        shutil.copy2(built, dst)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def build_hip(force=False, verbose=False):
    """Compile the reference's four extensions for gfx950 (no GPU needed).  Returns {ext: path or None} and, under "<ext>_build" for an extension
    with a stand-in header, which attempt produced the file: "unmodified" or "with oracle/<header>" (+ the seconds), as hip_build_note gives it."""
    import time
    out = {}
    for ext, (modname, files) in HIP_EXTENSIONS.items():
        srcs = [os.path.join(REF_ROOT, ext, "src", f) for f in files]
        dst = hip_path(ext)
        header = STAND_IN.get(ext)
        if not all(os.path.exists(p) for p in srcs):
            out[ext] = dst if os.path.exists(dst) else None
        else:
            hdrs = [os.path.join(REF_ROOT, ext, "src", f) for f in os.listdir(os.path.join(REF_ROOT, ext, "src")) if f.endswith(".h")]
            deps = srcs + hdrs + [os.path.abspath(__file__)] + ([header] if header else [])
            if force or not os.path.exists(dst) or os.path.getmtime(dst) < max(os.path.getmtime(p) for p in deps):
                os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
                os.environ.setdefault("MAX_JOBS", "4")
                t0 = time.time()
                how = "unmodified"
                try:
                    _build_one(ext, modname, files, dst, verbose)
                except Exception as e:  # noqa: BLE001 -- whatever the toolchain raises for a failed compile
                    errors = [ln.strip() for ln in str(e).splitlines() if "error:" in ln]
                    # the stand-in answers ONE failure, the compiler refusing the call of the missing overload; anything else (no ninja, a full
                    # disk, an unreadable scratch directory, another compile error) is not its business and is raised as it came
                    if header is None or not any("atomicAdd" in ln for ln in errors):
                        raise
                    for line in errors[:3]:      # the compiler's own words for why
                        print(f"[ref_build] {ext}: {line}")
                    print(f"[ref_build] {ext}: the unmodified build failed; second attempt with -include {os.path.relpath(header, ROOT)}")
                    how = f"with {os.path.relpath(header, ROOT)} (the unmodified build failed: {errors[0].split('error:', 1)[1].strip()})"
                    _build_one(ext, modname, files, dst, verbose, include=header)
                if header:
                    with open(os.path.join(OUT_DIR, f"ref_{ext}.build.txt"), "w") as f:
                        f.write(f"{how}; {time.time() - t0:.0f} s\n")
            out[ext] = dst
        if header:
            out[ext + "_build"] = hip_build_note(ext) if out[ext] else None
            print(f"[ref_build] {ext}: {out[ext + '_build']}")
    return out


def load_hip(ext):
    """Import oracle/_ref/ref_<ext>.so as the reference's extension module (its own PyInit name); needs torch imported (libtorch symbols)."""
    import importlib.util
    import torch  # noqa: F401
    modname = HIP_EXTENSIONS[ext][0]
    spec = importlib.util.spec_from_file_location(modname, hip_path(ext))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load():
    """Import the built module (needs torch imported first for its symbols)."""
    import importlib.util
    import torch  # noqa: F401
    spec = importlib.util.spec_from_file_location("_palette_func", OUT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_hip(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
