"""ABI 9 on the host: the jitter field of the frame structs and pnr_present_frame's validation (no GPU needed: every check below returns before a launch)."""
import ctypes
import os
import subprocess

from palettenerf_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_abi_version_and_present_entry_point():
    lib = _lib.load()
    assert lib.pnr_abi_version() >= 9
    assert _lib.SIGNATURES["pnr_present_frame"] == [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.pnr_present_frame(None, None) == -1
    a = _lib.PresentArgs()
    assert lib.pnr_present_frame(ctypes.byref(a), None) == 0          # an empty frame: nothing is read, nothing is launched
    a.dst_h, a.dst_w = 4, 6
    a.image = a.depth = a.out_image = a.out_depth = 8
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1         # a zero source size
    a.src_h, a.src_w = 2, 3
    a.out_image = None
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1         # a missing output
    a.out_image, a.out_depth = 8, None
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1
    a.out_depth, a.image = 8, None
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1         # a missing input
    a.image, a.out_xyz = 8, 8
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1         # the xyz map without rays / depth_origin
    a.out_xyz, a.out_clip = None, 8
    assert lib.pnr_present_frame(ctypes.byref(a), None) == -1         # the clip_feat map without its source
    a.dst_h = 0
    assert lib.pnr_present_frame(ctypes.byref(a), None) == 0


def test_frame_structs_carry_noises_behind_depth_raw():
    names = [f[0] for f in _lib.NerfFrameArgs._fields_]
    assert names[-2:] == ["depth_raw", "noises"] and _lib.NerfFrameArgs().noises is None
    base, pal = _lib.NerfFrameArgs, _lib.PaletteFrameArgs
    assert base.noises.offset == base.depth_raw.offset + ctypes.sizeof(ctypes.c_void_p)
    assert pal._fields_[0][0] == "base" and pal.base.offset == 0
    assert pal.embeddings_palette.offset == ctypes.sizeof(base)       # the palette struct's own fields still follow the (grown) base
    later = [f[0] for f in pal._fields_[1:]]
    assert later == ["embeddings_palette", "embeddings_clip", "num_basis", "clip_dim", "pred_clip", "offsets_weight", "view_dep_weight", "aux_map",
                     "embeddings_pair", "embeddings_triple", "edit"]
    offs = [getattr(pal, n).offset for n in later]
    assert offs == sorted(offs) and offs[0] >= base.noises.offset + ctypes.sizeof(ctypes.c_void_p)


def test_new_struct_layouts_are_the_headers(tmp_path):
    """pnr_present_args and the grown frame structs as gcc lays the header out (tests/test_abi.py does this for the older structs)."""
    pairs = {"pnr_present_args": _lib.PresentArgs, "pnr_nerf_frame_args": _lib.NerfFrameArgs, "pnr_palette_frame_args": _lib.PaletteFrameArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {']
    for cname, mirror in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, *_ in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for fname, *_ in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, f"{cname}.{fname}"
    assert len(_lib.PresentArgs._fields_) == 19
