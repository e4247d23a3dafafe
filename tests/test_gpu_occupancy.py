"""SURVEY section 8 f1 on the GPU: the device-resident occupancy sweep (csrc/occupancy.hip) against
  * what the REFERENCE's own update_extra_state / mark_untrained_grid drew, queried and left behind (tests/golden/occupancy.npz), and
  * the C oracle at the full 2 x 128^3 size.
Integer work (cells, Morton order, occupied list, bitfield away from the threshold) is bit-exact; the densities go through the exact-fp32
matrix path and agree with the CPU arithmetic to 2e-5 relative (reduction order, device exp)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import _lib, network, raymarching, scene

pytestmark = pytest.mark.gpu

SIGMA_RTOL = 2e-5
# The fixture's sigmas were computed by the reference on the CPU, where torch DIVIDES by (G - 1); a GPU -- the canonical form, which the kernel
# and the oracle restate -- multiplies by the fp32 reciprocal.  A third of the points differ by one ulp in some coordinate, and the finest
# hash-grid levels turn one ulp (2.4e-7 of a 4096-cell axis) into up to ~1e-4 of sigma.  The fixture records which points are identical: those
# are held to SIGMA_RTOL, the others to this.
ONE_ULP_POINT_RTOL = 3e-4


def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "occupancy.npz"))


def resize_grid(m, G):
    """The renderer hard-codes 128 as the reference does (nerf/renderer.py:85); every expression of the sweep is in terms of grid_size."""
    dev = m.density_grid.device
    m.grid_size = G
    m.density_grid = torch.zeros(m.cascade, G ** 3, device=dev)
    m.density_bitfield = torch.zeros(m.cascade * G ** 3 // 8, dtype=torch.uint8, device=dev)


def unpack(bits, C):
    return np.unpackbits(bits, bitorder="little").reshape(C, -1).astype(bool)


def assert_bitfield(got_bits, grid, thresh, C, rtol=SIGMA_RTOL):
    """got == (grid > thresh) except, at most, for cells whose density sits within rtol of the threshold."""
    want = grid > thresh
    diff = unpack(got_bits, C) ^ want
    near = np.abs(grid - thresh) <= rtol * np.abs(thresh)
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    return int(diff.sum())


def test_update_extra_state_replays_the_reference_fixture(cuda, golden_dir):
    g = fixture(golden_dir)
    G, C = int(g["G"]), 2
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=float(g["density_scale"]), min_near=0.2, density_thresh=1e9)
    scene.seed_field_(m, int(g["seed"]))
    m = m.to(cuda).train()
    resize_grid(m, G)
    assert m._fused_sweep_ok()
    # ---- full sweep: the reference's noise (stored by Morton index), its step counters
    m.local_step = 3
    m.step_counter[:3, 0] = torch.tensor([100, 200, 330], dtype=torch.int32, device=cuda)
    noise = torch.from_numpy(g["full_noise_u8"].astype(np.float32) / 256).to(cuda)
    m.update_extra_state(noise=noise)
    assert m.iter_density == 1 and m.local_step == 0 and m.mean_count == int(g["full_mean_count"]) == 210
    grid = m.density_grid.cpu().numpy()
    ref = g["full_grid"]
    same = np.unpackbits(g["full_points_same"])[:C * G ** 3].reshape(C, -1).astype(bool)
    rel = np.abs(grid / ref - 1)
    assert same.mean() > 0.5 and rel[same].max() < SIGMA_RTOL and rel.max() < ONE_ULP_POINT_RTOL, (rel[same].max(), rel.max())
    assert abs(m.mean_density / float(g["full_mean"]) - 1) < 1e-5
    # the bitfield is the packbits of the grid the kernel itself left, at the kernel's own mean -- exactly
    state_mean = np.float32(m.mean_density)
    assert np.array_equal(unpack(m.density_bitfield.cpu().numpy(), C), grid > state_mean)
    # and the reference's bitfield up to cells within the sigma tolerance of the mean
    d = unpack(m.density_bitfield.cpu().numpy(), C) ^ unpack(g["full_bitfield"], C)
    assert not (d & ~(np.abs(ref - float(g["full_mean"])) <= ONE_ULP_POINT_RTOL * ref)).any()
    # ---- partial sweep on the reference's state, with its draws
    m.density_grid.copy_(torch.from_numpy(g["part_before"]))
    m.iter_density, m.density_thresh = 16, float(g["part_density_thresh"])
    n = G ** 3 // 4
    coords = torch.from_numpy(g["part_coords_u8"].astype(np.int32)).to(cuda)
    occ_rand = torch.from_numpy(g["part_occ_rand"]).to(cuda)
    noise = torch.from_numpy(g["part_noise_u8"].astype(np.float32) / 256).to(cuda)
    m.update_extra_state(decay=float(g["part_decay"]), noise=noise, coords=coords, occ_rand=occ_rand)
    # expected: the oracle's commit (largest candidate per cell) of the REFERENCE's sigmas at the reference's points
    before = g["part_before"].copy()
    _, cells, p4 = oracle.occupancy_points(C, G, 2.0, g["part_noise_u8"].astype(np.float32) / 256, coords=g["part_coords_u8"].astype(np.int32),
                                           occ_rand=g["part_occ_rand"], density_grid=before, n_partial=n)
    want = before.copy()
    cand = (g["part_sigma"] * np.float32(g["density_scale"])).reshape(-1)
    wbits, wmean, wthresh = oracle.occupancy_commit(want, p4, cand, float(g["part_decay"]), float(g["part_density_thresh"]))
    grid = m.density_grid.cpu().numpy()
    live = want >= 0
    assert np.array_equal(grid[~live], want[~live])                                    # retired cells stay -1
    same = np.unpackbits(g["part_points_same"])[:C * 2 * n].astype(bool)
    all_same = np.ones(C * G ** 3, bool)
    np.logical_and.at(all_same, cells, same)            # cells all of whose candidates sit at identical points
    all_same = all_same.reshape(C, -1)
    rel = np.abs(grid / np.where(live, want, 1) - 1)
    assert rel[live & all_same].max() < SIGMA_RTOL and rel[live].max() < ONE_ULP_POINT_RTOL, (rel[live & all_same].max(), rel[live].max())
    assert abs(m.mean_density / wmean - 1) < 1e-5
    assert_bitfield(m.density_bitfield.cpu().numpy(), want, np.float32(wthresh), C, rtol=ONE_ULP_POINT_RTOL)
    assert np.array_equal(unpack(m.density_bitfield.cpu().numpy(), C), grid > np.float32(wthresh))     # exactly the packbits of the kernel's own grid
    assert m.iter_density == 17


def _points_of_sweep(m, mode_args):
    """All points of a sweep through pnr_occupancy_points (the kernel the fused call uses): float32 [n,4] on the host."""
    lib = _lib.load()
    a = _lib.OccupancyArgs()
    a.C, a.H, a.bound = m.cascade, m.grid_size, float(m.bound)
    a.density_grid = m.density_grid.data_ptr()
    a.mode, a.n_partial = mode_args["mode"], mode_args.get("n", 0)
    a.noise = mode_args["noise"].data_ptr()
    if a.mode == 1:
        a.coords, a.occ_rand = mode_args["coords"].data_ptr(), mode_args["occ_rand"].data_ptr()
    ws = torch.empty(int(lib.pnr_occupancy_workspace_bytes(a.C, a.H, 0)), dtype=torch.uint8, device=m.density_grid.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.pnr_occupancy_begin(ctypes.byref(a), stream), "begin")
    total = int(lib.pnr_occupancy_samples(ctypes.byref(a)))
    pts = torch.empty(total, 4, dtype=torch.float32, device=m.density_grid.device)
    _lib.check(lib.pnr_occupancy_points(ctypes.byref(a), 0, total, ctypes.c_void_p(pts.data_ptr()), stream), "points")
    torch.cuda.synchronize()
    return pts


def _oracle_sigma(m, xyz):
    """sigma of the field at world points on the CPU: oracle hash-grid lookup + fp32 fma-chain sigma_net + exp."""
    enc = m.encoder
    emb = enc.embeddings.detach().cpu().numpy()
    x01 = (xyz + np.float32(m.bound)) / np.float32(2 * m.bound)
    feat = oracle.grid_encode_forward(x01, emb, enc.offsets.cpu().numpy(), enc.per_level_scale, enc.base_resolution)   # [B, L*C]
    w0, w1 = m.sigma_net[0].weight.detach().cpu().numpy(), m.sigma_net[1].weight.detach().cpu().numpy()
    h = np.maximum(oracle.linear(feat, w0), 0)
    h0 = oracle.linear(h, np.ascontiguousarray(w1[:1]))[:, 0]
    return np.exp(h0.astype(np.float32))


def test_full_size_sweep_against_the_oracle(cuda):
    """2 x 128^3: points bit-exact against the oracle AND against the reference's torch expressions evaluated by torch on this GPU;
    densities 2e-5; bitfield identical away from the threshold, and exactly identical when the threshold sits in a gap of the densities."""
    G, C = 128, 2
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=0.7, min_near=0.2, density_thresh=1e9)
    scene.seed_field_(m, 5)
    m = m.to(cuda).train()
    torch.manual_seed(11)
    noise = torch.rand(C, G ** 3, 3, device=cuda)
    pts = _points_of_sweep(m, {"mode": 0, "noise": noise})
    hp = pts.cpu().numpy()
    oxyz, ocells, op4 = oracle.occupancy_points(C, G, 2.0, noise.cpu().numpy())
    assert np.array_equal(hp.view(np.int32), op4.view(np.int32))                 # bit for bit, ids included
    # the reference's expressions (nerf/renderer.py:484-499), by torch, on this device, cells visited in the reference's meshgrid order
    ax = torch.arange(G, dtype=torch.int32, device=cuda)
    coords = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    idx = raymarching.morton3D(coords).long()
    for cas in range(C):
        bound = min(2 ** cas, m.bound)
        half = bound / G
        xyzs = 2 * coords.float() / (G - 1) - 1
        cas_xyzs = xyzs * (bound - half)
        cas_xyzs += (noise[cas, idx] * 2 - 1) * half
        assert torch.equal(cas_xyzs, pts[cas * G ** 3 + idx, :3]), cas
    # the sweep itself
    with torch.cuda.device(cuda):
        torch.cuda.set_sync_debug_mode("error")      # any host wait inside the call raises
        try:
            m.update_extra_state(noise=noise)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    sub = np.arange(0, C * G ** 3, 7)                 # every 7th cell through the CPU arithmetic: 600 k samples
    want = _oracle_sigma(m, oxyz[sub]) * np.float32(0.7)
    grid = m.density_grid.cpu().numpy().reshape(-1)
    rel = np.abs(grid[sub] / want - 1).max()
    assert rel < SIGMA_RTOL, rel
    mean = np.float32(m.mean_density)
    assert abs(float(mean) / float(grid.astype(np.float64).mean()) - 1) < 1e-6
    bits = m.density_bitfield.cpu().numpy()
    assert np.array_equal(unpack(bits, 1)[0], grid > mean)
    # the mip the call rebuilt is the mip of that bitfield
    mip = raymarching.occupancy_mip(m.density_bitfield, C, G, m.bound)
    fresh = torch.empty_like(mip)
    _lib.call("pnr_build_occupancy_mip", ctypes.c_void_p(m.density_bitfield.data_ptr()), ctypes.c_uint32(C), ctypes.c_uint32(G), ctypes.c_float(m.bound),
              ctypes.c_void_p(fresh.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(mip, fresh)
    # EMA, mean, threshold and packbits alone, exactly: the oracle's commit of the kernel's own densities, with density_thresh below the
    # mean (so min(mean, density_thresh) takes the other branch) -> bit-identical bitfield
    thresh = np.float32(np.quantile(grid, 0.4))
    assert thresh < mean
    m2 = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=0.7, min_near=0.2, density_thresh=float(thresh))
    scene.seed_field_(m2, 5)
    m2 = m2.to(cuda).train()
    m2.update_extra_state(noise=noise)
    assert torch.equal(m2.density_grid, m.density_grid)        # deterministic: same inputs, same grid
    g2 = np.zeros((C, G ** 3), np.float32)
    ob, omean, oth = oracle.occupancy_commit(g2, op4, grid.copy(), 0.95, float(thresh))
    assert oth == thresh and np.array_equal(ob, m2.density_bitfield.cpu().numpy())
    assert abs(m2.mean_density - omean) <= 1e-7 * omean


@pytest.mark.parametrize("bound", [1.5, 3.0])
def test_small_sweep_at_a_bound_that_is_no_power_of_two(cuda, bound):
    """C x 32^3 at bound 1.5 (two cascades) and 3 (three): k_occ_lookup takes the division branch of unit_cube_of (grid_xside.hpp) and the last
    cascade's cells are bound / G wide, not 2^c / G.  The checks of test_full_size_sweep_against_the_oracle, on every cell: points bit for bit
    against the oracle, densities to SIGMA_RTOL, the bitfield the packbits of the kernel's own grid and the oracle's away from the threshold."""
    G = 32
    density_scale = 0.7
    m = network.NeRFNetwork(bound=bound, cuda_ray=True, density_scale=density_scale, min_near=0.2, density_thresh=1e9)
    C = m.cascade
    assert C == (2 if bound == 1.5 else 3)
    scene.seed_field_(m, 5)
    m = m.to(cuda).train()
    resize_grid(m, G)
    assert m._fused_sweep_ok()
    noise = torch.rand(C, G ** 3, 3, device=cuda, generator=torch.Generator(device="cuda").manual_seed(11))
    pts = _points_of_sweep(m, {"mode": 0, "noise": noise})
    oxyz, ocells, op4 = oracle.occupancy_points(C, G, bound, noise.cpu().numpy())
    assert np.array_equal(pts.cpu().numpy().view(np.int32), op4.view(np.int32))
    assert float(np.abs(oxyz).max()) > (1.0 if bound == 1.5 else 2.0) and float(np.abs(oxyz).max()) <= bound      # the last cascade spans the bound, not 2^c
    m.update_extra_state(noise=noise)
    want = (_oracle_sigma(m, oxyz) * np.float32(density_scale)).reshape(C, -1)
    grid = m.density_grid.cpu().numpy()
    cells = op4[:, 3].view(np.int32)
    assert np.array_equal(np.sort(cells), np.arange(C * G ** 3))             # a full sweep: one point per cell
    want_grid = np.empty(C * G ** 3, np.float32)
    want_grid[cells] = want.reshape(-1)
    rel = np.abs(grid.reshape(-1) / want_grid - 1).max()
    print(f"bound {bound}: densities within {rel:.3g} of the CPU arithmetic")
    assert rel < SIGMA_RTOL, rel
    mean = np.float32(m.mean_density)
    assert abs(float(mean) / float(grid.astype(np.float64).mean()) - 1) < 1e-6
    bits = m.density_bitfield.cpu().numpy()
    assert np.array_equal(unpack(bits, C), grid > mean)
    assert_bitfield(bits, want_grid.reshape(C, -1), mean, C)
    mip = raymarching.occupancy_mip(m.density_bitfield, C, G, m.bound)
    fresh = torch.empty_like(mip)
    _lib.call("pnr_build_occupancy_mip", ctypes.c_void_p(m.density_bitfield.data_ptr()), ctypes.c_uint32(C), ctypes.c_uint32(G), ctypes.c_float(m.bound),
              ctypes.c_void_p(fresh.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(mip, fresh)


def test_partial_sweep_occupied_list_and_duplicates(cuda):
    """mode 1 at full size with the draws made here: the occupied list is torch.nonzero's, repeated cells keep their largest candidate,
    cascades without an occupied cell skip the occupied half, nothing waits for the device."""
    G, C = 128, 2
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1.0, min_near=0.2, density_thresh=0.01)
    scene.seed_field_(m, 8)
    m = m.to(cuda).train()
    gen = torch.Generator(device="cuda").manual_seed(3)
    grid0 = torch.rand(C, G ** 3, device=cuda, generator=gen) - 0.6      # 40 % occupied, the rest <= 0
    grid0[1] = -0.25                                                    # cascade 1: nothing occupied
    grid0[0, 1000:1100] = -1.0
    m.density_grid.copy_(grid0)
    n = G ** 3 // 4
    coords = torch.randint(0, G, (C, n, 3), device=cuda, dtype=torch.int32, generator=gen)
    coords[0, :5000] = coords[0, 5000:10000]                            # guaranteed repeats
    occ_rand = torch.randint(0, 2 ** 31 - 1, (C, n), device=cuda, dtype=torch.int32, generator=gen)
    noise = torch.rand(C, 2 * n, 3, device=cuda, generator=gen)
    pts = _points_of_sweep(m, {"mode": 1, "n": n, "noise": noise, "coords": coords, "occ_rand": occ_rand}).cpu().numpy()
    oxyz, ocells, op4 = oracle.occupancy_points(C, G, 2.0, noise.cpu().numpy(), coords=coords.cpu().numpy(), occ_rand=occ_rand.cpu().numpy(),
                                                density_grid=grid0.cpu().numpy(), n_partial=n)
    assert np.array_equal(pts.view(np.int32), op4.view(np.int32))
    ids = pts[:, 3].view(np.int32).reshape(C, 2 * n)
    occ = torch.nonzero(grid0[0] > 0).squeeze(-1)
    assert np.array_equal(ids[0, n:], occ[(occ_rand[0].long() % occ.numel())].cpu().numpy())     # = occ_indices[rand_mask], renderer.py:520-522
    assert (ids[1, n:] == -1).all() and (ids[1, :n] >= G ** 3).all()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.iter_density = 16
        m.update_extra_state(noise=noise, coords=coords, occ_rand=occ_rand)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    live = ocells >= 0
    sig = np.zeros(ocells.shape[0], np.float32)
    pick = np.nonzero(live)[0][::5]
    sig[pick] = _oracle_sigma(m, oxyz[pick])
    grid = m.density_grid.cpu().numpy().reshape(-1)
    g0 = grid0.cpu().numpy().reshape(-1)
    # per drawn cell: new = max(old * decay, largest candidate) where old >= 0; check on the subsample that the kernel's value is >= every
    # candidate's EMA (to tolerance) and that cells drawn exactly once equal theirs
    cnt = np.bincount(ocells[live], minlength=C * G ** 3)
    ema = np.maximum(g0[ocells[pick]] * np.float32(0.95), sig[pick])
    updatable = g0[ocells[pick]] >= 0
    assert (grid[ocells[pick]][updatable] >= ema[updatable] * (1 - SIGMA_RTOL)).all()
    single = updatable & (cnt[ocells[pick]] == 1)
    assert single.sum() > 10000
    assert np.abs(grid[ocells[pick]][single] / ema[single] - 1).max() < SIGMA_RTOL
    untouched = np.ones(C * G ** 3, bool)
    untouched[ocells[live]] = False
    assert np.array_equal(grid[untouched], g0[untouched])     # cells not drawn keep their value: no decay either (renderer.py:541-542)
    assert np.array_equal(grid[g0 < 0], g0[g0 < 0])
    mean = np.float32(m.mean_density)
    thresh = min(mean, np.float32(0.01))
    assert np.array_equal(unpack(m.density_bitfield.cpu().numpy(), 1)[0], grid > thresh)


def test_generic_field_path_equals_the_fused_sweep(cuda):
    """A field without a fused kernel goes points -> its own density() -> scatter -> commit; with the shipped field forced down that road
    (torch sigma_net) the result must agree with the fused sweep to the sigma tolerance."""
    out = []
    for generic in (False, True):
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1.0, min_near=0.2)
        scene.seed_field_(m, 21)
        m = m.to(cuda).train()
        m.occupancy_generic = generic
        assert m._fused_sweep_ok() == (not generic)
        torch.manual_seed(77)
        noise = torch.rand(2, 128 ** 3, 3, device=cuda)
        m.update_extra_state(noise=noise)
        out.append((m.density_grid.clone(), m.density_bitfield.clone(), m.mean_density))
    (a, ba, ma), (b, bb, mb) = out
    assert float((a > 0).float().mean()) > 0.5
    assert float(((a - b).abs() / a.abs().clamp(min=1e-12)).max()) < SIGMA_RTOL
    thresh = min(ma, 0.01)
    near = int(((a - thresh).abs() <= SIGMA_RTOL * a.abs()).sum())
    assert int((ba ^ bb).to(torch.int32).ne(0).sum()) <= near


@pytest.mark.parametrize("filt", [False, True])
def test_mark_untrained_grid_against_fixture_and_oracle(cuda, golden_dir, filt):
    g = fixture(golden_dir)
    G, C = int(g["G"]), 2
    m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.2).to(cuda)
    m.filter_close_point = filt
    resize_grid(m, G)
    n = m.mark_untrained_grid(g["mark_poses"], tuple(float(v) for v in g["mark_intrinsics"]))
    ref = np.unpackbits(g["mark_grid_filter_close" if filt else "mark_grid"])[:C * G ** 3].reshape(C, -1).astype(bool)
    got = m.density_grid.cpu().numpy()
    assert np.array_equal(got < 0, ref) and int(n) == int(ref.sum())
    assert set(np.unique(got)) <= {-1.0, 0.0}
    # full size, 150 cameras (more than one LDS tile would need > 512: 600 here), against the oracle bit for bit
    m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.3).to(cuda)
    m.filter_close_point = filt
    rng = np.random.default_rng(4)
    poses = np.stack([scene.lookat_pose(radius=float(rng.uniform(0.5, 4.0)), elevation_deg=float(rng.uniform(-30, 60)), azimuth_deg=float(rng.uniform(0, 360)))
                      for _ in range(600)]).astype(np.float32)
    intr = (700.0, 720.0, 400.0, 380.0)
    n = m.mark_untrained_grid(poses, intr)
    want = np.zeros((C, 128 ** 3), np.float32)
    on = oracle.mark_untrained_grid(poses, intr, want, 2.0, 0.3, filt)
    assert int(n) == on and np.array_equal(m.density_grid.cpu().numpy(), want)
