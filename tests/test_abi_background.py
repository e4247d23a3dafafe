"""ABI 10 on the host: pnr_background_pack / pnr_background_forward and their argument struct (no GPU needed: every check below returns before a launch)."""
import ctypes
import os
import subprocess

from palettenerf_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def supported():
    a = _lib.BackgroundArgs()
    a.num_levels, a.level_dim, a.sh_degree, a.num_layers, a.hidden_dim = 4, 2, 4, 2, 64
    return a


def test_abi_version_is_10_and_the_entry_points_exist():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    assert _lib.SIGNATURES["pnr_background_forward"] == [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["pnr_background_pack"] == [ctypes.c_void_p] * 4
    assert lib.pnr_background_packed_bytes() == (64 * 24 + 64 * 4) * 4


def test_struct_layout_is_the_headers(tmp_path):
    cname, mirror = "pnr_background_args", _lib.BackgroundArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, *_ in mirror._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(mirror)
    for fname, *_ in mirror._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, fname
    assert len(mirror._fields_) == 21
    # the frame structs did not move: the background goes in through bg_map, as a per-ray colour
    assert [f[0] for f in _lib.NerfFrameArgs._fields_][-2:] == ["depth_raw", "noises"]


def test_null_and_unsupported_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -4
    assert lib.pnr_background_forward(None, None) == INVALID
    assert lib.pnr_background_forward(ctypes.byref(_lib.BackgroundArgs()), None) == UNSUPPORTED      # an all-zero architecture
    for field, bad in (("num_levels", 16), ("level_dim", 4), ("sh_degree", 3), ("num_layers", 3), ("hidden_dim", 32), ("table_dtype", 2), ("gridtype", 2)):
        a = supported()
        a.N = 8
        setattr(a, field, bad)
        assert lib.pnr_background_forward(ctypes.byref(a), None) == UNSUPPORTED, field
    a = supported()
    assert lib.pnr_background_forward(ctypes.byref(a), None) == 0            # N = 0: nothing to do, nothing is read
    a.N = 8
    assert lib.pnr_background_forward(ctypes.byref(a), None) == INVALID      # no pointers at all
    names = ("rays_o", "rays_d", "embeddings", "offsets", "packed", "out")
    for missing in names:
        a = supported()
        a.N, a.table_rows = 8, 64
        for n in names:
            setattr(a, n, None if n == missing else 256)
        assert lib.pnr_background_forward(ctypes.byref(a), None) == INVALID, missing
    a = supported()
    a.N = 8
    for n in names:
        setattr(a, n, 256)
    assert lib.pnr_background_forward(ctypes.byref(a), None) == INVALID      # table_rows = 0
    a.table_rows, a.packed = 64, 260
    assert lib.pnr_background_forward(ctypes.byref(a), None) == ALIGNMENT    # the blob is read 16 bytes at a time
    a.packed, a.coords_out = 256, 260
    assert lib.pnr_background_forward(ctypes.byref(a), None) == ALIGNMENT
    assert lib.pnr_background_pack(None, 256, 256, None) == INVALID
    assert lib.pnr_background_pack(256, 256, None, None) == INVALID
    assert lib.pnr_background_pack(256, 256, 260, None) == ALIGNMENT
