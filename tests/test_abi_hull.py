"""include/pnr_hull.h held the way tests/test_abi.py holds include/pnr.h: the entry is declared, bound (palettenerf_amd._lib.HULL_SIGNATURES,
beside SIGNATURES, which stays as it is) and exported, the ABI version is unchanged, the ctypes mirror has the size and every field offset gcc
gives the header's struct, and every refusal returns its code before a launch.  No GPU: the pointers are dummies that nothing may follow."""
import ctypes
import os
import re
import subprocess

from palettenerf_amd import _lib

INVALID, OK = -1, 0
P = 64      # a non-null, 16-byte aligned address that is never read
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "pnr_hull.h")


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", src)))


def hull_args(**over):
    a = _lib.HullSimplifyArgs()
    a.centers = a.center_weights = a.palette = a.info = a.errors = a.trace = a.vertices = P
    a.K, a.error_thres, a.target_size = 40, 5 / 255, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_entry_is_declared_bound_and_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    assert header_symbols() == sorted(_lib.HULL_SIGNATURES) == ["pnr_hull_simplify"]
    assert not set(_lib.HULL_SIGNATURES) & set(_lib.SIGNATURES)
    assert re.search(r"\bint pnr_hull_simplify\(const pnr_hull_simplify_args\* args, pnr_stream_t stream\);", open(HEADER).read())
    assert '#include "pnr.h"' in open(HEADER).read()
    fn = lib.pnr_hull_simplify
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_void_p] and fn.restype is ctypes.c_int
    assert "pnr_hull_simplify" not in open(os.path.join(INCLUDE, "pnr.h")).read().replace("pnr_hull.h", "")      # pnr.h only points to the header


def test_the_constants_are_the_headers():
    header = open(HEADER).read()
    for macro, value in (("PNR_HULL_MAX_M", _lib.HULL_MAX_M), ("PNR_HULL_MAX_RELATED", _lib.HULL_MAX_RELATED), ("PNR_HULL_OK", _lib.HULL_OK),
                         ("PNR_HULL_COPLANAR", _lib.HULL_COPLANAR), ("PNR_HULL_FLAT", _lib.HULL_FLAT), ("PNR_HULL_DENSE", _lib.HULL_DENSE)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    for i, rule in enumerate(("NONE", "ERROR", "TARGET", "UNCHANGED", "FOUR")):
        assert re.search(r"#define PNR_HULL_STOP_%s %d\b" % (rule, i), header), rule
    assert _lib.HULL_STOP == ("none", "error", "target", "unchanged", "four")
    assert re.search(r"#define PNR_HULL_ERROR_NONE \(-1\.0\)", header) and _lib.HULL_ERROR_NONE == -1.0
    assert re.search(r"#define PNR_HULL_ERROR_FAIL \(-2\.0\)", header) and _lib.HULL_ERROR_FAIL == -2.0
    assert _lib.HULL_MAX_RELATED >= 32 and _lib.HULL_MAX_M == _lib.LUT_MAX_M         # the issue's floor for the cap; a palette the LUT takes


def test_the_struct_mirror_has_the_layout_gcc_gives_the_header_struct(tmp_path):
    mirror = _lib.HullSimplifyArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr_hull.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(pnr_hull_simplify_args));']
    lines += [f'  printf("{f[0]} %zu\\n", offsetof(pnr_hull_simplify_args, {f[0]}));' for f in mirror._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.check_call(["gcc", "-I", INCLUDE, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])     # (a field the header lacks fails to compile)
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(mirror)
    for f in mirror._fields_:
        assert int(got[f[0]]) == getattr(mirror, f[0]).offset, f[0]
    # ... and the header has no field the mirror lacks
    body = re.search(r"typedef struct pnr_hull_simplify_args \{(.*?)\} pnr_hull_simplify_args;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]", "", n) for n in re.sub(r"^(const\s+)?\w+[\s\*]+", "", decl).split(",")]
    assert names == [f[0] for f in mirror._fields_]


def test_the_entry_refuses_before_a_launch():
    fn = _lib.load().pnr_hull_simplify
    assert fn(None, None) == INVALID
    for name in ("centers", "center_weights", "palette", "info"):
        assert fn(ctypes.byref(hull_args(**{name: None})), None) == INVALID, name
    for K in (0, 1, 3, _lib.EXTRACT_MAX_K + 1, 1 << 20):
        assert fn(ctypes.byref(hull_args(K=K)), None) == INVALID, K
    for thres in (-1e-9, -1.0, float("nan"), float("-inf")):
        assert fn(ctypes.byref(hull_args(error_thres=thres)), None) == INVALID, thres
    for target in (1, 2, 3, _lib.HULL_MAX_M + 1, 1 << 16):
        assert fn(ctypes.byref(hull_args(target_size=target)), None) == INVALID, target
    for name in ("centers", "center_weights", "palette", "errors", "vertices"):
        assert fn(ctypes.byref(hull_args(**{name: P + 4})), None) == INVALID, name           # float64 arrays: 8 bytes
    for name in ("info", "trace"):
        assert fn(ctypes.byref(hull_args(**{name: P + 2})), None) == INVALID, name           # int32 arrays: 4 bytes
    # the optional arrays may be absent, the limits of K and of target_size are accepted: none of these is refused for its arguments (they
    # would launch, so they are not called here); the struct's defaults above are such a call
