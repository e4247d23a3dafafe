"""Mesh export on the GPU: marching cubes of csrc/mesh.hip against the numpy statement of tests/mesh_reference.py -- vertices and triangles
equal BIT FOR BIT, order included -- the lattice points against the numpy formula, and the path from a model to a .ply file."""
import ctypes

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, mesh, network, scene
from tests import mesh_reference as ref

pytestmark = pytest.mark.gpu


def sphere(R):
    g = ref.lattice_axis(-1.0, 1.0, R)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return (np.float32(10) + np.float32(40) * (np.float32(0.6) - np.sqrt(X * X + Y * Y + Z * Z))).astype(np.float32), 10.0


def bordered_noise():
    u = np.random.default_rng(1).standard_normal((20, 20, 20)).astype(np.float32)
    u[0] = u[-1] = u[:, 0] = u[:, -1] = u[:, :, 0] = u[:, :, -1] = -5
    return u, 0.0


def open_noise():
    return np.random.default_rng(2).standard_normal((7, 18, 65)).astype(np.float32), 0.25      # non-cubic, open boundary, one point past 64


def blobs():
    g = np.linspace(-1, 1, 130, dtype=np.float32)                                                # 130^3 = 8583 blocks of 256 + a ragged end
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    u = np.zeros_like(X)
    for cx, cy, cz, s in ((-0.4, -0.3, 0.1, 0.30), (0.45, 0.2, -0.35, 0.25), (0.0, 0.55, 0.5, 0.2)):
        u += np.exp(-((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) / np.float32(s * s)).astype(np.float32)
    return u.astype(np.float32), 0.5


def on_threshold():
    u = np.random.default_rng(3).integers(-2, 3, size=(11, 12, 13)).astype(np.float32)          # a fifth of the values ARE the threshold
    return u, 0.0


def non_finite():
    rng = np.random.default_rng(4)
    u = rng.standard_normal((10, 9, 14)).astype(np.float32)
    k = rng.integers(0, 3, size=u.shape)
    u[(k == 0) & (rng.random(u.shape) < 0.2)] = np.inf
    u[(k == 1) & (rng.random(u.shape) < 0.2)] = np.nan
    u[(k == 2) & (rng.random(u.shape) < 0.1)] = -np.inf
    return u, 0.1


def checkerboard():
    i, j, k = np.meshgrid(*[np.arange(9)] * 3, indexing="ij")
    return (1.0 - 2.0 * ((i + j + k) & 1)).astype(np.float32), 0.0                               # every lattice edge straddles


FIELDS = {"sphere33": sphere, "bordered_noise": bordered_noise, "open_noise": open_noise, "blobs130": blobs, "on_threshold": on_threshold,
          "non_finite": non_finite, "checkerboard": checkerboard}
_expected = {}


def expected(name):
    """(u, threshold, V, T) of a field: the numpy statement, computed once and shared."""
    if name not in _expected:
        u, thr = (sphere(33) if name == "sphere33" else FIELDS[name]())
        V, T = ref.marching_cubes(u, thr)
        for a in (u, V, T):
            a.setflags(write=False)
        _expected[name] = (u, thr, V, T)
    return _expected[name]


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_equals_the_numpy_statement_bit_for_bit(cuda, name):
    u, thr, V, T = expected(name)
    v, t = mesh.marching_cubes(torch.tensor(u, device=cuda), thr)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    v, t = v.cpu().numpy(), t.cpu().numpy()
    print(name, "vertices", len(V), "triangles", len(T))
    assert v.shape == V.shape and t.shape == T.shape
    assert np.array_equal(t, T)
    assert np.array_equal(v.view(np.uint32), V.view(np.uint32))
    v2, t2 = mesh.marching_cubes(torch.tensor(u, device=cuda), thr)                               # a second run: the same bits
    assert np.array_equal(v2.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(t2.cpu().numpy(), t)
    if name == "checkerboard":
        assert len(V) == 3 * 9 * 9 * 8                                                            # every edge of the lattice
    if name in ("sphere33", "bordered_noise", "blobs130"):
        ref.assert_closed(v, t, euler=2 if name == "sphere33" else None)
    if name == "blobs130":
        # the blobs span more than 80 x-planes of 130 * 130 points, i.e. of 66 workgroups of 256 consecutive points each: the vertices' ranks
        # come from at least that many different block offsets of the scan
        point = (np.floor(v[:, 0]) * 130 + np.floor(v[:, 1])) * 130 + np.floor(v[:, 2])
        assert len(np.unique(point.astype(np.int64) // 256)) >= 80


def test_numpy_in_gives_numpy_out(cuda):
    u, thr, V, T = expected("open_noise")
    v, t = mesh.marching_cubes(u, thr)
    assert isinstance(v, np.ndarray) and isinstance(t, np.ndarray) and np.array_equal(v, V) and np.array_equal(t, T)


@pytest.mark.parametrize("value", [-1.0, 1.0])
def test_a_field_without_a_surface_gives_an_empty_mesh(cuda, value):
    u = torch.full((9, 17, 70), value, device=cuda)
    v, t = mesh.marching_cubes(u, 0.0)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
    torch.cuda.synchronize()


def test_short_output_buffers_are_not_overrun(cuda):
    """pnr_mesh_emit writes no row at or past the capacities it is given."""
    u, thr, V, T = expected("bordered_noise")
    ud = torch.tensor(u, device=cuda)
    lib = _lib.load()
    need = int(lib.pnr_mesh_workspace_bytes(*u.shape))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    counts = torch.zeros(2, dtype=torch.int32, device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.pnr_mesh_count(ud.data_ptr(), *u.shape, thr, ws.data_ptr(), need, counts.data_ptr(), stream), "count")
    assert counts.cpu().tolist() == [len(V), len(T)]
    cv, ct = len(V) // 2, len(T) // 3
    v = torch.full((len(V), 3), -7.0, device=cuda)
    t = torch.full((len(T), 3), -7, dtype=torch.int32, device=cuda)
    _lib.check(lib.pnr_mesh_emit(ud.data_ptr(), *u.shape, thr, ws.data_ptr(), need, v.data_ptr(), cv, t.data_ptr(), ct, stream), "emit")
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert np.array_equal(v[:cv], V[:cv]) and (v[cv:] == -7).all()
    assert np.array_equal(t[:ct], T[:ct]) and (t[ct:] == -7).all()


def test_lattice_points_equal_the_numpy_formula_bit_for_bit(cuda):
    lo, hi, n = (-1.25, 0.1, -3.0), (0.75, 0.9, 5.5), (5, 6, 33)
    want = ref.lattice(lo, hi, n)
    total = len(want)
    whole = mesh.lattice_points(lo, hi, n, 0, total, cuda).cpu().numpy()
    assert np.array_equal(whole.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(whole[-1], np.asarray(hi, np.float32)) and np.array_equal(whole[0], np.asarray(lo, np.float32))
    for first, count in ((1, 300), (257, 700), (total - 5, 5), (500, 1)):
        part = mesh.lattice_points(lo, hi, n, first, count, cuda).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), want[first:first + count].view(np.uint32)), first


def shipped_model(cuda, seed=5):
    m = network.NeRFNetwork(bound=1, cuda_ray=True)
    scene.seed_field_(m, seed)
    return m.to(cuda).eval()


def exact_density(m, pts):
    """DensityFused at precision 0 on grid_encode_raw at the points: the exact-fp32 path the occupancy sweep is already held equal to."""
    from palettenerf_amd.fused import DensityFused
    d = DensityFused(m)
    d.precision = 0
    return d(pts, want_geo=False)[0]


def second_trip_resolution():
    """The smallest cubic lattice whose single chunk sends workgroups of the capped sigma_net launch on a second trip through their tile loop."""
    cap, rpt = _lib.launch_geometry("pnr_lattice_density", 1 << 31)
    R = 2
    while R ** 3 <= cap * rpt:
        R += 1
    wg, rpt = _lib.launch_geometry("pnr_lattice_density", R ** 3)
    assert R ** 3 > wg * rpt and R ** 3 <= mesh.LATTICE_CHUNK            # one chunk, more tiles than workgroups
    return R


@pytest.mark.parametrize("R", [20, None])
def test_the_fused_lattice_density_equals_the_exact_density_path_bit_for_bit(cuda, R):
    """pnr_lattice_density over the whole aabb_infer: the top plane sits exactly on +bound (one ulp further and the encoder reads zero)."""
    R = R or second_trip_resolution()
    m = shipped_model(cuda)
    assert m._fused_sweep_ok()
    u = mesh.lattice_density(m, m.aabb_infer[:3], m.aabb_infer[3:], R)
    assert u.is_cuda and tuple(u.shape) == (R, R, R) and u.dtype == torch.float32
    pts = torch.from_numpy(ref.lattice([-1.0] * 3, [1.0] * 3, (R, R, R))).to(cuda)
    want = exact_density(m, pts).reshape(R, R, R)
    assert torch.equal(u, want)
    outside = float(exact_density(m, torch.full((1, 3), 1.5, device=cuda))[0])               # what a point out of range reads
    top = u[-1].cpu().numpy()
    assert np.isfinite(top).all() and (top != outside).mean() > 0.99 and top.std() > 0
    assert torch.equal(mesh.lattice_density(m, m.aabb_infer[:3], m.aabb_infer[3:], R), u)    # a second run: the same bits
    if R == 20:                                                                               # several chunks with a ragged last one: the same volume
        old, mesh.LATTICE_CHUNK = mesh.LATTICE_CHUNK, 3072
        try:
            assert torch.equal(mesh.lattice_density(m, m.aabb_infer[:3], m.aabb_infer[3:], R), u)
        finally:
            mesh.LATTICE_CHUNK = old


def test_a_replaced_density_is_asked_not_bypassed(cuda):
    """An instance-level density() turns the fused call off (renderer._fused_sweep_ok): the volume is what that density() returns, chunk by chunk."""
    m = shipped_model(cuda)
    m.density = lambda x: {"sigma": x[:, 0] + 2 * x[:, 1] + 4 * x[:, 2]}
    old, mesh.LATTICE_CHUNK = mesh.LATTICE_CHUNK, 1000
    try:
        u = mesh.lattice_density(m, resolution=(5, 6, 33))
    finally:
        mesh.LATTICE_CHUNK = old
    p = ref.lattice([-1.0] * 3, [1.0] * 3, (5, 6, 33))
    want = torch.from_numpy(p).to(cuda)
    assert torch.equal(u.reshape(-1), want[:, 0] + 2 * want[:, 1] + 4 * want[:, 2])


def test_a_generic_field_from_density_to_ply(cuda, tmp_path):
    """An instance-level density(): the analytic sphere |x| = 0.5 as sigma = 10 + 40 (0.5 - |x|)."""
    m = network.NeRFNetwork(bound=1, cuda_ray=True).to(cuda).eval()
    m.density = lambda x: {"sigma": 10 + 40 * (0.5 - x.norm(dim=-1))}
    R = 24
    v, t = mesh.extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], R, 10, model=m)
    assert v.dtype == np.float64 and t.dtype == np.int32 and len(t) > 500
    h = 2.0 / (R - 1)
    assert np.abs(np.linalg.norm(v, axis=1) - 0.5).max() < h
    ref.assert_closed(v, t, euler=2)
    u = mesh.extract_fields(m.aabb_infer[:3], m.aabb_infer[3:], R, lambda p: m.density(p)["sigma"])
    assert isinstance(u, np.ndarray) and u.shape == (R, R, R) and u.dtype == np.float32
    path = str(tmp_path / "meshes" / "sphere.ply")
    v2, t2 = mesh.save_mesh(m, path, resolution=R, threshold=10)
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    vr, tr = mesh.read_ply(path)
    assert np.array_equal(vr, v.astype(np.float32)) and np.array_equal(tr, t)
