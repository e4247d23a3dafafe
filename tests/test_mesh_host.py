"""The mesh export's conventions on the host (no GPU): the numpy statement of tests/mesh_reference.py with the library's case table on fields
whose surface is known, the lattice formula against torch.linspace, and the PLY writer."""
import numpy as np
import pytest
import torch

from palettenerf_amd import mesh
from tests import mesh_reference as ref

TABLE = ref.case_table()


def grid(R, lo=-1.0, hi=1.0):
    g = ref.lattice_axis(lo, hi, R)
    return np.meshgrid(g, g, g, indexing="ij")


def sphere_field(R, r=0.6):
    X, Y, Z = grid(R)
    return (np.float32(10) + np.float32(40) * (np.float32(r) - np.sqrt(X * X + Y * Y + Z * Z))).astype(np.float32)


@pytest.mark.parametrize("R,lowest", [(17, 0.96), (33, 0.99)])
def test_sphere_is_closed_oriented_and_inscribed(R, lowest):
    """u = 10 + 40 (0.6 - |x|) over [-1, 1]^3 at threshold 10: the sphere |x| = 0.6.  Vertices lie on lattice edges at the linearly interpolated
    crossing of a field that is concave along every line, hence inside the sphere: the mesh is inscribed and its volume stays below the
    sphere's.  Measured with this table: 0.9747 at R = 17, 0.9936 at R = 33."""
    V, T = ref.marching_cubes(sphere_field(R), 10.0, TABLE)
    r = ref.assert_closed(V, T, euler=2)
    h = 2.0 / (R - 1)
    ratio = r["volume"] * h ** 3 / (4.0 / 3.0 * np.pi * 0.6 ** 3)
    print("R", R, "vertices", len(V), "triangles", len(T), "volume / analytic", ratio)
    assert lowest <= ratio < 1.0, ratio                         # positive: normals point out of the dense region


def test_torus_has_euler_characteristic_zero():
    X, Y, Z = grid(40)
    u = (0.04 - ((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)).astype(np.float32)
    V, T = ref.marching_cubes(u, 0.0, TABLE)
    r = ref.assert_closed(V, T, euler=0)
    assert r["volume"] > 0


def test_noise_with_a_border_is_closed():
    rng = np.random.default_rng(0)
    u = rng.standard_normal((12, 12, 12)).astype(np.float32)
    u[0] = u[-1] = u[:, 0] = u[:, -1] = u[:, :, 0] = u[:, :, -1] = -5
    V, T = ref.marching_cubes(u, 0.0, TABLE)
    assert len(T) > 100
    ref.assert_closed(V, T)


@pytest.mark.parametrize("lo,hi,n", [(-1.0, 1.0, 256), (-24.0, 24.0, 256), (0.1, 0.9, 130), (-2.0, 2.0, 33), (-1.0, 1.0, 2), (-0.7, 1.3, 5),
                                     (3.0, -3.0, 64)])
def test_lattice_formula_against_torch_linspace(lo, hi, n):
    got = ref.lattice_axis(lo, hi, n)
    want = torch.linspace(lo, hi, n, dtype=torch.float32).numpy()
    assert got.dtype == np.float32 and got[0] == np.float32(lo) and got[-1] == np.float32(hi)          # endpoints exact
    ulp = np.spacing(np.float32(max(abs(lo), abs(hi))))
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= ulp
    if lo < hi:
        assert (np.diff(got) > 0).all()


def test_ply_round_trip(tmp_path):
    V, T = ref.marching_cubes(sphere_field(9), 10.0, TABLE)
    path = str(tmp_path / "sphere.ply")
    mesh.write_ply(path, V.astype(np.float64), T.astype(np.int64))          # what extract_geometry hands over: float64 vertices
    head = open(path, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    V2, T2 = mesh.read_ply(path)
    assert V2.dtype == np.float32 and T2.dtype == np.int32
    assert np.array_equal(V2, V) and np.array_equal(T2, T)
    import os
    assert os.path.getsize(path) == head.index(b"end_header\n") + 11 + len(V) * 12 + len(T) * 13
    empty = str(tmp_path / "empty.ply")
    mesh.write_ply(empty, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    V0, T0 = mesh.read_ply(empty)
    assert V0.shape == (0, 3) and T0.shape == (0, 3) and V0.dtype == np.float32 and T0.dtype == np.int32
