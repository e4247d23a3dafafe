"""The marching-cubes case table of csrc/mesh.hip (generated: csrc/gen_mc_tables.py), read through pnr_mesh_case_triangles, against the cube's
geometry -- all 256 cases, no GPU.  What is proved here holds for any field: a cell's patch is closed up to its faces, and the two cells that
share a face draw the same segments on it in opposite directions, so the surface is watertight and consistently oriented."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from palettenerf_amd import _lib
from tests import mesh_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID = -1
TABLE = ref.case_table()


def straddling(case):
    return {e for e in range(12) if ((case >> ref.edge_corners(e)[0]) ^ (case >> ref.edge_corners(e)[1])) & 1}


def in_one_face(e0, e1):
    pts = [ref.corner_xyz(c) for e in (e0, e1) for c in ref.edge_corners(e)]
    return any(len({int(p[d]) for p in pts}) == 1 for d in range(3))


def directed(case):
    return [(t[k], t[(k + 1) % 3]) for t in TABLE[case] for k in range(3)]


def boundary(case):
    """Directed triangle edges whose reverse is not in the patch: the patch's rim."""
    d = directed(case)
    return [e for e in d if (e[1], e[0]) not in d]


def test_counts():
    assert TABLE[0] == [] and TABLE[255] == []
    assert max(len(t) for t in TABLE) == 5 and sum(len(t) for t in TABLE) == 820
    assert all(len(TABLE[c]) >= 1 for c in range(1, 255))


@pytest.mark.parametrize("case", range(256))
def test_a_case_uses_exactly_its_straddling_edges_and_closes_up_to_the_faces(case):
    tris = TABLE[case]
    assert {e for t in tris for e in t} == straddling(case)
    assert all(len(set(t)) == 3 for t in tris)
    d = directed(case)
    assert len(d) == len(set(d))                                   # no directed edge twice
    for e0, e1 in d:
        if (e1, e0) in d:
            assert not in_one_face(e0, e1), (case, e0, e1)         # an interior edge (a fan diagonal) never lies in a face
        else:
            assert in_one_face(e0, e1), (case, e0, e1)             # the rim lies in the cube's faces


def face_segments(case, axis, side):
    """Rim segments of a case that lie in the face `axis = side`, as pairs of in-face edge names (edge axis, offsets on the face's two axes)."""
    out = set()
    for e0, e1 in boundary(case):
        names = []
        for e in (e0, e1):
            c0, c1 = (ref.corner_xyz(c) for c in ref.edge_corners(e))
            if c0[axis] != side or c1[axis] != side:
                break
            others = [d for d in range(3) if d != axis]
            names.append((ref.EDGES[e][0], int(c0[others[0]]), int(c0[others[1]])))
        else:
            out.add(tuple(names))
    return out


@pytest.mark.parametrize("axis", range(3))
def test_faces_agree_across_cells(axis):
    """For each 4-corner sign pattern of a face: every case with that pattern draws the same segments on it, and the + face's segments are the
    reverses of the - face's (the neighbouring cell sees the same face from the other side)."""
    others = [d for d in range(3) if d != axis]
    seen = {0: {}, 1: {}}
    for case in range(256):
        for side in (0, 1):
            pattern = 0
            for k, (p, q) in enumerate(itertools.product((0, 1), repeat=2)):
                v = [0, 0, 0]
                v[axis], v[others[0]], v[others[1]] = side, p, q
                pattern |= ((case >> (v[0] + 2 * v[1] + 4 * v[2])) & 1) << k
            segs = face_segments(case, axis, side)
            assert seen[side].setdefault(pattern, segs) == segs, (case, side, pattern)
    assert len(seen[0]) == len(seen[1]) == 16
    for pattern in range(16):
        assert seen[1][pattern] == {(b, a) for a, b in seen[0][pattern]}, pattern
        crossings = sum(1 for a, b in ((0, 1), (1, 3), (3, 2), (2, 0)) if ((pattern >> a) ^ (pattern >> b)) & 1)
        assert len(seen[0][pattern]) == crossings // 2


def test_case_1_points_out_of_the_dense_corner():
    (tri,) = TABLE[1]
    mid = [sum(ref.corner_xyz(c) for c in ref.edge_corners(e)) / 2.0 for e in tri]
    n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    assert (n > 0).all(), n


def test_the_committed_table_is_what_the_generator_gives():
    import importlib.util
    path = os.path.join(ROOT, "palettenerf_amd", "csrc", "gen_mc_tables.py")
    spec = importlib.util.spec_from_file_location("gen_mc_tables", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert [[tuple(t) for t in case] for case in gen.table()] == TABLE


def test_entries_are_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pnr_lattice_points", "pnr_lattice_density", "pnr_lattice_density_workspace_bytes", "pnr_mesh_case_triangles", "pnr_mesh_workspace_bytes", "pnr_mesh_count", "pnr_mesh_emit"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pnr_abi_version() == 10


def test_arguments_outside_the_contract_are_refused_before_any_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)         # never dereferenced: every call below must return before it touches the device
    assert lib.pnr_mesh_case_triangles(256, None) == INVALID and lib.pnr_mesh_case_triangles(7, None) == len(TABLE[7])
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (513, 8, 8), (8, 513, 8), (8, 8, 513), (0, 0, 0)):
        assert lib.pnr_mesh_workspace_bytes(*dims) == 0
        assert lib.pnr_mesh_count(fake, *dims, 0.0, fake, 1 << 40, fake, None) == INVALID
        assert lib.pnr_mesh_emit(fake, *dims, 0.0, fake, 1 << 40, fake, 1, fake, 1, None) == INVALID
    need = lib.pnr_mesh_workspace_bytes(8, 9, 10)
    assert need >= 8 * 9 * 10 * 4 and lib.pnr_mesh_workspace_bytes(512, 512, 512) >= 4 * 512 ** 3
    assert lib.pnr_mesh_workspace_bytes(512, 512, 512) < 4.1 * 512 ** 3          # ~4 bytes per lattice point
    assert lib.pnr_mesh_count(None, 8, 9, 10, 0.0, fake, need, fake, None) == INVALID
    assert lib.pnr_mesh_count(fake, 8, 9, 10, 0.0, None, need, fake, None) == INVALID
    assert lib.pnr_mesh_count(fake, 8, 9, 10, 0.0, fake, need, None, None) == INVALID
    assert lib.pnr_mesh_count(fake, 8, 9, 10, 0.0, fake, need - 1, fake, None) == INVALID
    assert lib.pnr_mesh_count(fake, 8, 9, 10, 0.0, ctypes.c_void_p(0x1010), need, fake, None) == INVALID      # workspace not 256-byte aligned
    assert lib.pnr_mesh_emit(None, 8, 9, 10, 0.0, fake, need, fake, 1, fake, 1, None) == INVALID
    assert lib.pnr_mesh_emit(fake, 8, 9, 10, 0.0, None, need, fake, 1, fake, 1, None) == INVALID
    assert lib.pnr_mesh_emit(fake, 8, 9, 10, 0.0, fake, need - 1, fake, 1, fake, 1, None) == INVALID
    assert lib.pnr_mesh_emit(fake, 8, 9, 10, 0.0, fake, need, None, 1, fake, 1, None) == INVALID
    assert lib.pnr_mesh_emit(fake, 8, 9, 10, 0.0, fake, need, fake, 1, None, 1, None) == INVALID
    assert lib.pnr_mesh_emit(fake, 8, 9, 10, 0.0, fake, need, None, 0, None, 0, None) == 0                    # an empty surface: nothing to write
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    n = (ctypes.c_uint32 * 3)(4, 5, 6)
    assert lib.pnr_lattice_points(lo, hi, n, 0, 0, fake, None) == 0
    assert lib.pnr_lattice_points(None, hi, n, 0, 1, fake, None) == INVALID
    assert lib.pnr_lattice_points(lo, None, n, 0, 1, fake, None) == INVALID
    assert lib.pnr_lattice_points(lo, hi, None, 0, 1, fake, None) == INVALID
    assert lib.pnr_lattice_points(lo, hi, n, 0, 1, None, None) == INVALID
    assert lib.pnr_lattice_points(lo, hi, n, 120, 1, fake, None) == INVALID and lib.pnr_lattice_points(lo, hi, n, 100, 21, fake, None) == INVALID
    for bad in ((1, 5, 6), (4, 513, 6)):
        assert lib.pnr_lattice_points(lo, hi, (ctypes.c_uint32 * 3)(*bad), 0, 1, fake, None) == INVALID


def test_lattice_density_refuses_arguments_outside_the_contract_before_any_launch():
    lib = _lib.load()
    UNSUPPORTED = -2

    def args(**kw):
        a = _lib.LatticeDensityArgs()
        for d in range(3):
            a.box_min[d], a.box_max[d], a.n[d] = -1.0, 1.0, 8
        a.bound, a.num_levels, a.S, a.base_resolution, a.gridtype = 1.0, 16, 0.5, 16, 0
        a.embeddings = a.offsets = a.packed_sigma_net = a.u = 0x1000                 # never dereferenced
        a.workspace, a.workspace_bytes = 0x1000, lib.pnr_lattice_density_workspace_bytes(256)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.pnr_lattice_density_workspace_bytes(256) == 256 * 144 and lib.pnr_lattice_density_workspace_bytes(257) == 512 * 144
    assert lib.pnr_lattice_density(None, None) == INVALID
    for field in ("embeddings", "offsets", "packed_sigma_net", "u", "workspace"):
        assert lib.pnr_lattice_density(ctypes.byref(args(**{field: None})), None) == INVALID, field
    assert lib.pnr_lattice_density(ctypes.byref(args(workspace_bytes=256 * 144 - 1)), None) == INVALID       # room for fewer than 256 points
    assert lib.pnr_lattice_density(ctypes.byref(args(workspace=0x1010)), None) == INVALID                    # not 256-byte aligned
    for n in ((1, 8, 8), (8, 8, 513)):
        a = args()
        for d in range(3):
            a.n[d] = n[d]
        assert lib.pnr_lattice_density(ctypes.byref(a), None) == INVALID, n
    assert lib.pnr_lattice_density(ctypes.byref(args(num_levels=8)), None) == UNSUPPORTED
    assert lib.pnr_lattice_density(ctypes.byref(args(gridtype=2)), None) == UNSUPPORTED
    assert lib.pnr_lattice_density(ctypes.byref(args(bound=0.0)), None) == UNSUPPORTED


def test_the_capped_sigma_launch_of_the_density_lattice_reports_its_geometry():
    cap, rpt = _lib.launch_geometry("pnr_lattice_density", 1 << 31)
    assert cap >= 1 and rpt >= 1
    for rows in (1, rpt, rpt + 1, 8000, cap * rpt, cap * rpt + 1, 1 << 22):
        assert _lib.launch_geometry("pnr_lattice_density", rows) == (min(-(-rows // rpt), cap), rpt)
    assert (cap * rpt + 1) ** (1 / 3) < 128          # a lattice small enough for a quick test reaches the second trip
