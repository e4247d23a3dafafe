"""GPU parity tests proper: every HIP kernel, called through the C ABI (via the operator mirror),
against the CPU oracle on the same seeded inputs.  Integer / index / count outputs must be
bit-exact; fp32 outputs carry the tolerance written next to each assertion."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import gridencoder, palette_utils, raymarching, scene, shencoder
from tests import float64_blocks as f64

pytestmark = pytest.mark.gpu

EXP_TOL = dict(rtol=2e-5, atol=2e-6)  # __expf (v_exp_f32) vs libm expf in the compositing kernels


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def s0():
    grid = scene.brick_density_grid()
    return grid, scene.packbits_np(grid, 0.5)


def rays_of(H, W, elev=30.0, azim=45.0):
    pose = torch.from_numpy(scene.lookat_pose(elevation_deg=elev, azimuth_deg=azim))[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro[0].numpy(), rd[0].numpy()


# ------------------------------------------------------------------------------------------ integer / utils
def test_morton_bit_exact(cuda):
    rng = np.random.default_rng(0)
    c = rng.integers(0, 1024, size=(100003, 3)).astype(np.int32)
    idx = raymarching.morton3D(dev(c, cuda))
    np.testing.assert_array_equal(host(idx), oracle.morton3D(c))
    np.testing.assert_array_equal(host(raymarching.morton3D_invert(idx)), c)
    full = np.stack(np.meshgrid(*[np.arange(128, dtype=np.int32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    got = host(raymarching.morton3D(dev(full, cuda)))
    np.testing.assert_array_equal(got, oracle.morton3D(full))
    assert np.array_equal(np.sort(got), np.arange(128 ** 3))  # full-size sweep is a bijection
    assert raymarching.morton3D(torch.zeros(0, 3, dtype=torch.int32, device=cuda)).shape == (0,)


def test_packbits_bit_exact(cuda, s0):
    grid, bf = s0
    got = raymarching.packbits(dev(grid, cuda), 0.5)
    np.testing.assert_array_equal(host(got), bf)
    rng = np.random.default_rng(1)
    g = rng.random((2, 128 ** 3)).astype(np.float32)
    buf = torch.zeros(2 * 128 ** 3 // 8, dtype=torch.uint8, device=cuda)
    out = raymarching.packbits(dev(g, cuda), 0.37, buf)
    assert out.data_ptr() == buf.data_ptr()  # writes into the given buffer
    np.testing.assert_array_equal(host(out), oracle.packbits(g, 0.37))


def test_near_far_bit_exact(cuda):
    rng = np.random.default_rng(2)
    o = rng.uniform(-3, 3, (50001, 3)).astype(np.float32)
    d = rng.standard_normal((50001, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0.0  # axis-aligned rays: 1/dx = inf
    o[:50, 0] = 2.0   # origin exactly on a slab with dx = 0: 0*inf NaNs
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    n, f = raymarching.near_far_from_aabb(dev(o, cuda), dev(d, cuda), dev(aabb, cuda), 0.05)
    on, of = oracle.near_far_from_aabb(o, d, aabb, 0.05)
    np.testing.assert_array_equal(host(n), on)
    np.testing.assert_array_equal(host(f), of)


def test_sph_from_ray(cuda):
    rng = np.random.default_rng(3)
    o = rng.uniform(-0.5, 0.5, (1000, 3)).astype(np.float32)
    d = rng.standard_normal((1000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    got = host(raymarching.sph_from_ray(dev(o, cuda), dev(d, cuda), 2.5))
    np.testing.assert_allclose(got, oracle.sph_from_ray(o, d, 2.5), atol=2e-6)  # atan2f/sqrtf implementations differ by ulps


# ------------------------------------------------------------------------------------------ march
@pytest.fixture(params=["mip", "nomip"])
def mip_mode(request):
    """Every march test runs through both kernel variants: occupancy mip in LDS, and plain global probes."""
    old = raymarching.USE_MIP
    raymarching.USE_MIP = request.param == "mip"
    yield request.param
    raymarching.USE_MIP = old


def test_occupancy_mip_matches_numpy(cuda, s0):
    grid, bf = s0
    rng = np.random.default_rng(77)
    bf2 = bf.copy()
    bf2[rng.integers(0, bf2.size, 5000)] = 0xFF
    bf2[:64] = 0xFF
    t = dev(bf2, cuda)
    mip = raymarching.occupancy_mip(t, 2, 128, 2.0)
    words = bf2.view(np.uint64)
    any_bits = np.packbits(words != 0, bitorder="little").view(np.uint32)
    all_bits = np.packbits(words == np.uint64(0xFFFFFFFFFFFFFFFF), bitorder="little").view(np.uint32)
    got = host(mip).view(np.uint32)
    np.testing.assert_array_equal(got[:2048], any_bits)
    np.testing.assert_array_equal(got[2048:4096], all_bits)
    box = got[4096:4102].view(np.float32)
    assert np.all(box[:3] <= -2.0) and np.all(box[3:] >= 2.0)  # bricks set at random all over the volume: the box covers it
    s0box = host(raymarching.occupancy_mip(dev(bf, cuda), 2, 128, 2.0)).view(np.uint32)[4096:4102].view(np.float32)
    np.testing.assert_allclose(s0box, [-0.8125] * 3 + [0.8125] * 3, atol=1e-6)  # S0: bricks of cascade 1 reach +-0.75, plus two 1/32 cells
    assert raymarching.occupancy_mip(t, 2, 128, 2.0) is mip          # cached
    t.bitwise_or_(torch.tensor(1, dtype=torch.uint8, device=cuda))  # torch in-place write bumps the version -> rebuilt
    assert raymarching.occupancy_mip(t, 2, 128, 2.0) is not mip
    # the cache entry lives on the tensor object: a NEW tensor that gets the freed tensor's address (what the caching allocator does when a
    # model is dropped and another one built) starts without a mip, whatever its version counter says
    addr = t.data_ptr()
    del t, mip
    bf3 = bf.copy()
    bf3[100000:100064] = 0xFF
    t3 = dev(bf3, cuda)
    got3 = host(raymarching.occupancy_mip(t3, 2, 128, 2.0)).view(np.uint32)
    np.testing.assert_array_equal(got3[:2048], np.packbits(bf3.view(np.uint64) != 0, bitorder="little").view(np.uint32))
    assert addr  # (t3 usually sits at `addr` again; the check above holds either way)


@pytest.mark.parametrize("dt_gamma,min_near,bound", [(0.0, 0.2, 2.0), (1.0 / 128, 0.02, 2.0), (1.0 / 256, 0.05, 1.5)])
def test_march_rays_train_bit_exact(cuda, s0, mip_mode, dt_gamma, min_near, bound, monkeypatch):
    """Both second passes: the rows written from the stored sample parameters (default) and the second walk (k_march_train_write: t_store off,
    which T_STORE_MAX = 0 forces) must equal the oracle bit for bit, with and without the mip, for both counting passes."""
    _march_rays_train_bit_exact(cuda, s0, dt_gamma, min_near, bound, monkeypatch, 64, 48)


@pytest.mark.parametrize("bound", [2.0, 1.5])
def test_march_rays_train_bit_exact_four_rays_per_wave(cuda, s0, mip_mode, bound, monkeypatch):
    """More than 8192 rays: the cooperative counting pass takes four rays per wave (k_march_train_count_coop<.., .., 4>), one instantiation per
    (mip, power-of-two bound).  96 x 96 rays; the checks of test_march_rays_train_bit_exact."""
    _march_rays_train_bit_exact(cuda, s0, 0.0, 0.2, bound, monkeypatch, 96, 96)


def _march_rays_train_bit_exact(cuda, s0, dt_gamma, min_near, bound, monkeypatch, H, W):
    grid, bf = s0
    ro, rd = rays_of(H, W)
    N = ro.shape[0]
    aabb = np.array([-bound, -bound, -bound, bound, bound, bound], np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, min_near)
    cnt = np.zeros(2, np.int32)
    ox, od, odl, orays = oracle.march_rays_train(ro, rd, bound, bf, 2, 128, on, of, cnt, align=128, force_all_rays=True, dt_gamma=dt_gamma)
    assert int(cnt[0]) > 10000
    from palettenerf_amd import _lib
    lib = _lib.load()
    try:
        for coop, t_store in ((1, True), (0, True), (1, False), (0, False)):   # the counting pass: a wave per ray (or four) cooperatively (k_march_train_count_coop) / one ray per lane
            assert lib.pnr_set_option(b"train_coop", coop) == 0
            monkeypatch.setattr(raymarching, "T_STORE_MAX", 1 << 26 if t_store else 0)
            counter = torch.zeros(2, dtype=torch.int32, device=cuda)
            x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), bound, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                          -1, False, 128, True, dt_gamma, 1024)
            np.testing.assert_array_equal(host(counter), cnt)            # total sample count and ray count: bit-exact
            np.testing.assert_array_equal(host(rays), orays)             # per-ray (id, offset, count): bit-exact, deterministic row order
            assert x.shape == ox.shape
            np.testing.assert_array_equal(host(x), ox)                   # positions bit-exact (canonical fmaf spec on both sides)
            np.testing.assert_array_equal(host(d), od)
            np.testing.assert_array_equal(host(dl), odl)
    finally:
        lib.pnr_set_option(b"train_coop", 1)


def test_march_rays_train_perturbed_and_mean_count_overflow(cuda, s0):
    grid, bf = s0
    ro, rd = rays_of(32, 32)
    N = ro.shape[0]
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.2)
    # a counter that does not start at zero: rows are offset by it, the rows in front and the alignment tail are zero (the outputs are
    # allocated uninitialised on this path, the kernel / the wrapper clear exactly those rows)
    cnt = np.array([300, 0], np.int32)
    ox, od, odl, orays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, on, of, cnt, align=128, force_all_rays=True)
    counter = torch.tensor([300, 0], dtype=torch.int32, device=cuda)
    torch.empty(N * 1024 * 3, device=cuda).fill_(7.0)            # dirty the allocator's blocks
    x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                  -1, False, 128, True, 0.0, 1024)
    np.testing.assert_array_equal(host(counter), cnt)
    np.testing.assert_array_equal(host(rays), orays)
    np.testing.assert_array_equal(host(x), ox)
    np.testing.assert_array_equal(host(d), od)
    np.testing.assert_array_equal(host(dl), odl)
    # overflow path: M = mean_count rounded up, rays that do not fit are dropped (raymarching.cu:419)
    cnt = np.zeros(2, np.int32)
    ox, od, odl, orays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, on, of, cnt, mean_count=5000, align=128)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                  5000, False, 128, False, 0.0, 1024)
    assert x.shape[0] == 5120 and int(counter[0]) > 5120
    np.testing.assert_array_equal(host(counter), cnt)
    np.testing.assert_array_equal(host(rays), orays)
    np.testing.assert_array_equal(host(x), ox)
    np.testing.assert_array_equal(host(dl), odl)
    # perturb=True draws torch.rand noises on the device: check counts stay within one step of the unperturbed march
    counter.zero_()
    _, _, _, rays_p = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                   -1, True, 128, True, 0.0, 1024)
    cnt2 = np.zeros(2, np.int32)
    _, _, _, rays0 = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, on, of, cnt2, align=128, force_all_rays=True)
    diff = np.abs(host(rays_p)[:, 2] - rays0[:, 2])  # a shift of the start by < one step moves a few cell crossings
    assert diff.max() <= 8 and diff.mean() < 1.0 and abs(int(counter[0]) - int(cnt2[0])) < 0.01 * int(cnt2[0])


def _far_rays(n, seed):
    """Cameras far outside the occupied cube of an S0 scene (bound 8): long empty walks in front of the box, which the
    GPU path jumps over exactly (csrc/march_core.hpp skip_to_box).  Mixed in: axis-parallel rays, rays that graze a
    face plane of the occupied box, rays that start inside it, rays that miss."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(3.0, 7.5, size=(n, 1))
    target = rng.uniform(-0.9, 0.9, size=(n, 3))
    k = n // 8
    target[:k, 2] = 0.8125                                   # on the +z face plane of the S0 box
    o[k:2 * k] = rng.uniform(-0.5, 0.5, size=(k, 3))         # inside the box
    target[2 * k:3 * k] = rng.uniform(2.0, 6.0, size=(k, 3))  # mostly misses
    d = target - o
    d[3 * k:4 * k, 0] = 0.0                                  # parallel to the x slabs
    d[4 * k:5 * k, :2] = 0.0; o[4 * k:5 * k, :2] = rng.uniform(-0.6, 0.6, size=(k, 2))  # straight down the z axis
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128, 1.0 / 32])
@pytest.mark.parametrize("perturb", [False, True])
def test_march_far_cameras_exact_empty_space_jump(cuda, dt_gamma, perturb):
    bound, C = 8.0, 4
    grid = scene.brick_density_grid(bound=8)
    bf = scene.packbits_np(grid, 0.5)
    ro, rd = _far_rays(6000, 5)
    N = ro.shape[0]
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.05)
    torch.manual_seed(77)
    noises = host(torch.rand(N, dtype=torch.float32, device=cuda)) if perturb else np.zeros(N, np.float32)
    cnt = np.zeros(2, np.int32)
    ox, od, odl, orays = oracle.march_rays_train(ro, rd, bound, bf, C, 128, on, of, cnt, noises=noises, align=128, force_all_rays=True, dt_gamma=dt_gamma)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    torch.manual_seed(77)
    x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), bound, dev(bf, cuda), C, 128, dev(on, cuda), dev(of, cuda), counter,
                                                  -1, perturb, 128, True, dt_gamma, 1024)
    assert int(cnt[0]) > 50000 and int((orays[:, 2] == 0).sum()) > 100
    np.testing.assert_array_equal(host(counter), cnt)
    np.testing.assert_array_equal(host(rays), orays)
    np.testing.assert_array_equal(host(x), ox)
    np.testing.assert_array_equal(host(dl), odl)       # delta[1] of a ray's first sample spans the jumped-over space
    # inference march from the same starts (n_step 2), half of the rays
    alive = np.arange(0, N, 2, dtype=np.int32)
    ix, idr, idl = oracle.march_rays(len(alive), 2, alive, on, ro, rd, bound, bf, C, 128, on, of, align=128, dt_gamma=dt_gamma)
    gx, gd, gdl = raymarching.march_rays(len(alive), 2, dev(alive, cuda), dev(on, cuda), dev(ro, cuda), dev(rd, cuda), bound, dev(bf, cuda), C, 128,
                                         dev(on, cuda), dev(of, cuda), 128, False, dt_gamma, 1024)
    np.testing.assert_array_equal(host(gx), ix)
    np.testing.assert_array_equal(host(gdl), idl)


@pytest.mark.parametrize("n_step,bound", [(1, 2.0), (3, 2.0), (8, 2.0), (4, 1.5)])
def test_march_rays_inference_bit_exact(cuda, s0, mip_mode, n_step, bound):
    grid, bf = s0
    ro, rd = rays_of(48, 40)
    N = ro.shape[0]
    aabb = np.array([-bound, -bound, -bound, bound, bound, bound], np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.2)
    rng = np.random.default_rng(4)
    alive = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    rays_t = on.copy()
    rays_t[alive[::3]] += 0.5  # some rays already advanced
    ox, od, odl = oracle.march_rays(len(alive), n_step, alive, rays_t, ro, rd, bound, bf, 2, 128, on, of, align=128, dt_gamma=1.0 / 256)
    # the wrapper hands the kernel UNINITIALISED buffers (pnr_march_rays_fill clears unfilled slots and the alignment rows itself): dirty the
    # allocator's blocks first so that a slot the kernel forgot cannot pass as the reference's zero-fill by luck
    for rows in (ox.shape[0] * 3, ox.shape[0] * 3, ox.shape[0] * 2):
        torch.empty(rows, device=cuda).fill_(float("nan"))
    from palettenerf_amd import _lib
    lib = _lib.load()
    try:
        for coop in (1, 0):   # the last rays of a wave marched by the whole wave (march_coop_tail) / every lane to the end of its own ray
            assert lib.pnr_set_option(b"coop_march", coop) == 0
            x, d, dl = raymarching.march_rays(len(alive), n_step, dev(alive, cuda), dev(rays_t, cuda), dev(ro, cuda), dev(rd, cuda), bound, dev(bf, cuda), 2, 128,
                                              dev(on, cuda), dev(of, cuda), 128, False, 1.0 / 256, 1024)
            assert x.shape == ox.shape and x.shape[0] % 128 == 0 and x.shape[0] > len(alive) * n_step - 1
            np.testing.assert_array_equal(host(x), ox)
            np.testing.assert_array_equal(host(d), od)
            np.testing.assert_array_equal(host(dl), odl)
    finally:
        lib.pnr_set_option(b"coop_march", 1)
    assert int((odl[:, 0] > 0).sum()) > 0


@pytest.mark.parametrize("n_rays,n_step,max_steps", [(1, 32, 1024), (3, 1, 1024), (5, 7, 64), (63, 16, 1024), (65, 2, 16), (130, 32, 1024)])
def test_march_kernels_cooperative_paths_on_tiny_and_ragged_batches(cuda, s0, n_rays, n_step, max_steps):
    """The wave-cooperative machinery of the drop-in march kernels at its edges: fewer rays than a wave's cooperative slots, a last wave with one ray,
    more samples per ray than a 16-lane window, a step budget below a window -- pnr_march_rays (cooperative tail) and pnr_march_rays_train (four rays
    per wave) against the oracle, bit for bit."""
    grid, bf = s0
    ro, rd = rays_of(16, 16, elev=20.0, azim=10.0)
    sel = np.linspace(0, ro.shape[0] - 1, n_rays).astype(np.int64)
    ro, rd = np.ascontiguousarray(ro[sel]), np.ascontiguousarray(rd[sel])
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.2)
    alive = np.arange(n_rays, dtype=np.int32)
    ox, od, odl = oracle.march_rays(n_rays, n_step, alive, on, ro, rd, 2.0, bf, 2, 128, on, of, align=128, dt_gamma=0.0, max_steps=max_steps)
    x, d, dl = raymarching.march_rays(n_rays, n_step, dev(alive, cuda), dev(on, cuda), dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128,
                                      dev(on, cuda), dev(of, cuda), 128, False, 0.0, max_steps)
    np.testing.assert_array_equal(host(x), ox)
    np.testing.assert_array_equal(host(d), od)
    np.testing.assert_array_equal(host(dl), odl)
    for dt_gamma in (0.0, 1.0 / 128):
        cnt = np.zeros(2, np.int32)
        tx, td, tdl, trays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, on, of, cnt, align=128, force_all_rays=True, dt_gamma=dt_gamma, max_steps=max_steps)
        counter = torch.zeros(2, dtype=torch.int32, device=cuda)
        gx, gd, gdl, grays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                          -1, False, 128, True, dt_gamma, max_steps)
        np.testing.assert_array_equal(host(counter), cnt)
        np.testing.assert_array_equal(host(grays), trays)
        np.testing.assert_array_equal(host(gx), tx)
        np.testing.assert_array_equal(host(gdl), tdl)


def test_compact_alive_is_stable_and_exact(cuda):
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 255, 256, 257, 100000, 640000):
        a = rng.integers(0, 1 << 20, n).astype(np.int32)
        a[rng.random(n) < 0.6] = -1
        out, count = raymarching.compact_alive(dev(a, cuda))
        k = int(count.item())
        want = a[a >= 0]
        assert k == len(want)
        np.testing.assert_array_equal(host(out)[:k], want)
    out, count = raymarching.compact_alive(dev(np.full(1000, -1, np.int32), cuda))
    assert int(count.item()) == 0


# ------------------------------------------------------------------------------------------ composite
def _train_case(rng, N, max_len, nc):
    counts = rng.integers(0, max_len, N)
    counts[:3] = 0
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts.sum())
    rays = np.stack([rng.permutation(N), offs, counts], 1).astype(np.int32)
    sig = (rng.random(M) * 40).astype(np.float32)
    rgb = rng.random((M, 3)).astype(np.float32)
    feat = rng.standard_normal((M, nc)).astype(np.float32)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    return rays, sig, rgb, feat, dl, M


@pytest.mark.parametrize("N,sigma_scale", [(300, 1.0), (3000, 1.0), (3000, 0.03)])
def test_composite_train_forward_backward(cuda, N, sigma_scale):
    """N = 300: the sample-order kernels (M < 65536); N = 3000: the 16-lanes-per-ray scan kernels, with opaque rays that stop at T_thresh
    after ~30 samples and with translucent ones that run their full length."""
    rng = np.random.default_rng(6)
    rays, sig, rgb, feat, dl, M = _train_case(rng, N, 200, 33)
    sig = (sig * sigma_scale).astype(np.float32)
    assert (M >= 65536) == (N == 3000)
    ts, tc = dev(sig, cuda).requires_grad_(True), dev(rgb, cuda).requires_grad_(True)
    ws, dep, img = raymarching.composite_rays_train(ts, tc, dev(dl, cuda), dev(rays, cuda), 1e-4)
    ows, odep, oimg = oracle.composite_rays_train_forward(sig, rgb, dl, rays, 1e-4)
    np.testing.assert_allclose(host(ws), ows, **EXP_TOL)
    np.testing.assert_allclose(host(dep), odep, **EXP_TOL)
    np.testing.assert_allclose(host(img), oimg, **EXP_TOL)
    gws, gimg = rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    ((ws * dev(gws, cuda)).sum() + (img * dev(gimg, cuda)).sum() + dep.sum()).backward()  # grad_depth is ignored by design
    ogs, ogc = oracle.composite_rays_train_backward(gws, gimg, sig, rgb, dl, rays, ows, oimg, 1e-4)
    np.testing.assert_allclose(host(tc.grad), ogc, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(host(ts.grad), ogs, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("nc", [1, 3, 16, 33, 128])
def test_composite_flex_train_forward_backward(cuda, nc):
    rng = np.random.default_rng(7)
    N = 1500
    rays, sig, rgb, feat, dl, M = _train_case(rng, N, 120, nc)
    tf = dev(feat, cuda).requires_grad_(True)
    out = raymarching.composite_rays_flex_train(dev(sig, cuda), tf, dev(dl, cuda), dev(rays, cuda), 1e-4)
    oout = oracle.composite_rays_flex_train_forward(sig, feat, dl, rays, 1e-4)
    np.testing.assert_allclose(host(out), oout, rtol=2e-5, atol=2e-5)
    go = rng.standard_normal((N, nc)).astype(np.float32)
    (out * dev(go, cuda)).sum().backward()
    np.testing.assert_allclose(host(tf.grad), oracle.composite_rays_flex_train_backward(go, sig, feat, dl, rays, 1e-4), rtol=2e-5, atol=2e-6)


def test_composite_flex_channel_limit(cuda):
    with pytest.raises(RuntimeError, match="unsupported"):
        raymarching.composite_rays_flex_train(torch.zeros(4, device=cuda), torch.zeros(4, 129, device=cuda), torch.zeros(4, 2, device=cuda),
                                              torch.zeros(1, 3, dtype=torch.int32, device=cuda), 1e-4)


@pytest.mark.parametrize("n_step", [1, 4, 8])
def test_composite_rays_inference_in_place(cuda, n_step):
    rng = np.random.default_rng(8)
    N, n_alive = 5000, 3100
    alive = np.sort(rng.choice(N, n_alive, replace=False)).astype(np.int32)
    M = n_alive * n_step
    sig = (rng.random(M) * 60).astype(np.float32)
    rgb = rng.random((M, 3)).astype(np.float32)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    dl[rng.random(M) < 0.1] = 0  # unfilled slots (delta == 0 sentinel)
    st = dict(rays_t=rng.random(N).astype(np.float32), ws=(rng.random(N) * 0.7).astype(np.float32), dep=rng.random(N).astype(np.float32),
              img=rng.random((N, 3)).astype(np.float32))
    feat = rng.standard_normal((M, 50)).astype(np.float32)
    out50 = rng.standard_normal((N, 50)).astype(np.float32)
    # oracle (flex first: it must see the weights_sum of BEFORE composite_rays)
    o_out = out50.copy()
    o = {k: v.copy() for k, v in st.items()}
    o_alive = alive.copy()
    oracle.composite_rays_flex(n_alive, n_step, 50, o_alive, o["rays_t"], sig, feat, dl, o["ws"], o_out, 1e-4)
    oracle.composite_rays(n_alive, n_step, o_alive, o["rays_t"], sig, rgb, dl, o["ws"], o["dep"], o["img"], 1e-4)
    g = {k: dev(v, cuda) for k, v in st.items()}
    g_alive, g_out = dev(alive, cuda), dev(out50, cuda)
    r = raymarching.composite_rays_flex(n_alive, n_step, 50, g_alive, g["rays_t"], dev(sig, cuda), dev(feat, cuda), dev(dl, cuda), g["ws"], g_out, 1e-4)
    assert r == tuple()
    np.testing.assert_array_equal(host(g["ws"]), st["ws"])  # flex never writes weights_sum / rays_alive / rays_t
    np.testing.assert_array_equal(host(g_alive), alive)
    raymarching.composite_rays(n_alive, n_step, g_alive, g["rays_t"], dev(sig, cuda), dev(rgb, cuda), dev(dl, cuda), g["ws"], g["dep"], g["img"], 1e-4)
    np.testing.assert_array_equal(host(g_alive), o_alive)      # which rays terminated: exact
    np.testing.assert_allclose(host(g_out), o_out, rtol=2e-5, atol=2e-5)
    for k in st:
        np.testing.assert_allclose(host(g[k]), o[k], **EXP_TOL)


@pytest.mark.parametrize("n_step", [1, 2, 5, 8, 11])
def test_composite_rays_flex_multi_is_bit_identical_to_the_single_calls(cuda, n_step):
    """SURVEY 8(b)'s multi-map variant (pnr_composite_rays_flex_multi): the seven flex composites of one PaletteNeRF march iteration (palette/renderer.py:508-516:
    3, 3, nb, 3 nb, 3 nb, clip_dim channels + a wide one) as one launch == the seven single launches bit for bit == the oracle (2e-5); dead slots, rays that
    cross T_thresh inside the run, n_step beyond the kernel's eight-step form (falls back to single launches), a zero-channel map, more than eight maps."""
    rng = np.random.default_rng(80 + n_step)
    N, n_alive = 4000, 2500
    alive = np.sort(rng.choice(N, n_alive, replace=False)).astype(np.int32)
    M = n_alive * n_step
    sig = (rng.random(M) * 90).astype(np.float32)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    dl[rng.random(M) < 0.12] = 0
    ws = (rng.random(N) * 1.0).astype(np.float32)            # some rays already past 1 - T_thresh
    chans = [3, 3, 4, 12, 12, 0, 16, 50, 1, 128]
    ins = [rng.standard_normal((M, max(c, 1))).astype(np.float32)[:, :c] for c in chans]
    outs = [rng.standard_normal((N, max(c, 1))).astype(np.float32)[:, :c] for c in chans]
    g_alive, g_ws, g_sig, g_dl = dev(alive, cuda), dev(ws, cuda), dev(sig, cuda), dev(dl, cuda)
    rays_t = torch.zeros(N, device=cuda)
    single = [dev(np.ascontiguousarray(o), cuda) for o in outs]
    g_ins = [dev(np.ascontiguousarray(i), cuda) for i in ins]
    for c, i, o in zip(chans, g_ins, single):
        if c:
            raymarching.composite_rays_flex(n_alive, n_step, c, g_alive, rays_t, g_sig, i, g_dl, g_ws, o, 1e-4)
    multi = [dev(np.ascontiguousarray(o), cuda) for o in outs]
    r = raymarching.composite_rays_flex_multi(n_alive, n_step, g_alive, rays_t, g_sig, g_dl, g_ws, list(zip(chans, g_ins, multi)), 1e-4)
    assert r == tuple()
    for c, a, b in zip(chans, single, multi):
        assert torch.equal(a, b), c
    # the single call itself runs on the cooperative kernel (n_step <= 8): the one-thread-per-ray kernel it replaced gives the same bits
    from palettenerf_amd import _lib as plib
    lib = plib.load()
    assert lib.pnr_set_option(b"flex_coop", 0) == 0
    try:
        for c, i, o, want in zip(chans, g_ins, outs, single):
            if c:
                plain = dev(np.ascontiguousarray(o), cuda)
                raymarching.composite_rays_flex(n_alive, n_step, c, g_alive, rays_t, g_sig, i, g_dl, g_ws, plain, 1e-4)
                assert torch.equal(plain, want), c
    finally:
        lib.pnr_set_option(b"flex_coop", 1)
    np.testing.assert_array_equal(host(g_ws), ws)
    np.testing.assert_array_equal(host(g_alive), alive)
    for m in (7, 8, 0):      # 50 channels, one channel, three
        o_out = np.ascontiguousarray(outs[m]).copy()
        oracle.composite_rays_flex(n_alive, n_step, chans[m], alive.copy(), np.zeros(N, np.float32), sig, np.ascontiguousarray(ins[m]), dl, ws.copy(), o_out, 1e-4)
        np.testing.assert_allclose(host(multi[m]), o_out, rtol=2e-5, atol=2e-5)
    with pytest.raises(RuntimeError, match="unsupported"):
        raymarching.composite_rays_flex_multi(n_alive, n_step, g_alive, rays_t, g_sig, g_dl, g_ws, [(129, g_ins[0], multi[0])], 1e-4)


def test_deferred_flex_composites_reach_the_device_as_one_launch_with_the_same_bits(cuda):
    """raymarching.arm_flex_deferral() (what dropin.fuse_field does behind every fused PaletteNetwork.forward): the flex composites that follow are queued and
    issued by the next composite_rays -- which must still see them done BEFORE it moves weights_sum -- as one pnr_composite_rays_flex_multi call; the deferral ends
    there (the next flex call is immediate again)."""
    from palettenerf_amd import _torch_glue
    rng = np.random.default_rng(91)
    N, n_alive, n_step = 3000, 1700, 4
    alive = np.sort(rng.choice(N, n_alive, replace=False)).astype(np.int32)
    M = n_alive * n_step
    sig, rgb = dev((rng.random(M) * 60).astype(np.float32), cuda), dev(rng.random((M, 3)).astype(np.float32), cuda)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    dl[rng.random(M) < 0.1] = 0
    dl = dev(dl, cuda)
    chans = [3, 3, 4, 12, 12, 16]
    ins = [dev(rng.standard_normal((M, c)).astype(np.float32), cuda) for c in chans]

    def state():
        g = torch.Generator().manual_seed(5)
        return dict(alive=dev(alive, cuda), t=torch.rand(N, generator=g).to(cuda), ws=(torch.rand(N, generator=g) * 0.7).to(cuda), dep=torch.rand(N, generator=g).to(cuda),
                    img=torch.rand(N, 3, generator=g).to(cuda), outs=[torch.rand(N, c, generator=g).to(cuda) for c in chans])

    def iteration(st, arm):
        if arm:
            raymarching.arm_flex_deferral()
        for c, i, o in zip(chans, ins, st["outs"]):
            assert raymarching.composite_rays_flex(n_alive, n_step, c, st["alive"], st["t"], sig, i, dl, st["ws"], o, 1e-4) == tuple()
        raymarching.composite_rays(n_alive, n_step, st["alive"], st["t"], sig, rgb, dl, st["ws"], st["dep"], st["img"], 1e-4)

    a, b = state(), state()
    iteration(a, False)
    prof = _torch_glue.profile_kernels(["pnr_composite_rays_flex", "pnr_composite_rays_flex_multi"])
    try:
        iteration(b, True)
        assert len(prof["pnr_composite_rays_flex"]) == 0 and len(prof["pnr_composite_rays_flex_multi"]) == 1
        out = torch.zeros(N, 3, device=cuda)        # the deferral has ended with composite_rays: an immediate call again
        f = state()                                 # (a fresh alive list: composite_rays has marked b's terminated rays with -1, as the reference does)
        raymarching.composite_rays_flex(n_alive, n_step, 3, f["alive"], f["t"], sig, ins[0], dl, f["ws"], out, 1e-4)
        assert len(prof["pnr_composite_rays_flex"]) == 1
    finally:
        _torch_glue.profile_kernels(None)
    for k in ("alive", "t", "ws", "dep", "img"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["outs"], b["outs"]):
        assert torch.equal(x, y)
    # the persistent switch, and a call whose shared arguments differ from the queue's flushes the queue first
    was = raymarching.defer_flex_composites(True)
    try:
        c, d = state(), state()
        raymarching.composite_rays_flex(n_alive, n_step, 3, c["alive"], c["t"], sig, ins[0], dl, c["ws"], c["outs"][0], 1e-4)
        raymarching.composite_rays_flex(n_alive, n_step, 3, d["alive"], d["t"], sig, ins[1], dl, d["ws"], d["outs"][1], 1e-4)     # another ray state: flushes c's
        raymarching.flush_flex_composites()
    finally:
        raymarching.defer_flex_composites(was)
    e = state()
    raymarching.composite_rays_flex(n_alive, n_step, 3, e["alive"], e["t"], sig, ins[0], dl, e["ws"], e["outs"][0], 1e-4)
    raymarching.composite_rays_flex(n_alive, n_step, 3, e["alive"], e["t"], sig, ins[1], dl, e["ws"], e["outs"][1], 1e-4)
    assert torch.equal(c["outs"][0], e["outs"][0]) and torch.equal(d["outs"][1], e["outs"][1])


def test_spread_ray_to_sample(cuda):
    rng = np.random.default_rng(9)
    N = 700
    rays, sig, rgb, feat, dl, M = _train_case(rng, N, 50, 3)
    inp = rng.random((N, 3)).astype(np.float32)
    out = torch.zeros(M, 3, device=cuda)
    raymarching.spread_ray_to_sample(dev(inp, cuda), dev(rays, cuda), out)
    want = np.zeros((M, 3), np.float32)
    oracle.spread_ray_to_sample(inp, rays, want)
    np.testing.assert_array_equal(host(out), want)


# ------------------------------------------------------------------------------------------ grid encoder
def _grid_setup(rng, L, H, log2T, desired, C, B):
    pls = float(np.exp2(np.log2(desired / H) / (L - 1))) if desired else 2.0
    offsets = oracle.grid_offsets(3, L, pls, H, log2T)
    emb = (rng.random((int(offsets[-1]), C)) - 0.5).astype(np.float32)
    x = rng.random((B, 3)).astype(np.float32)
    x[:5] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1.0000001, 0.5, 0.5], [-1e-7, 0.2, 0.3]]  # boundaries in, epsilon-outside out
    return pls, offsets, emb, x


@pytest.mark.parametrize("C", [1, 2, 4, 8])
def test_grid_encode_forward_fp32_bit_exact(cuda, C):
    rng = np.random.default_rng(10 + C)
    L = 16 if C == 2 else 6
    pls, offsets, emb, x = _grid_setup(rng, L, 16, 19 if C == 2 else 12, 4096 if C == 2 else None, C, 20011)
    out = gridencoder.grid_encode(dev(x, cuda), dev(emb, cuda), dev(offsets, cuda), pls, 16, False, 0, False)
    want = oracle.grid_encode_forward(x, emb, offsets, pls, 16)
    assert out.shape == (x.shape[0], L * C)
    np.testing.assert_array_equal(host(out), want)  # same fmaf chain, same host-computed level scales => bit-exact


def test_grid_encode_tiled_and_align_corners(cuda):
    rng = np.random.default_rng(20)
    pls, offsets, emb, x = _grid_setup(rng, 6, 8, 10, None, 2, 3001)
    for gridtype, ac in ((1, False), (0, True), (1, True)):
        out = gridencoder.grid_encode(dev(x, cuda), dev(emb, cuda), dev(offsets, cuda), pls, 8, False, gridtype, ac)
        np.testing.assert_array_equal(host(out), oracle.grid_encode_forward(x, emb, offsets, pls, 8, gridtype=gridtype, align_corners=ac))


@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
def test_grid_pair_lookup_with_align_corners_is_bit_identical_to_two_lookups(cuda, gridtype):
    """fused.grid_encode_raw_pair with align_corners=True -- the pair kernel's own branch, which no other test reaches -- against two single lookups
    and the oracle, bit for bit; the shapes of test_grid_encode_tiled_and_align_corners (6 levels, H = 8, 2^10 rows, 3001 points: the faces 0 and 1
    and points an epsilon outside among them)."""
    from palettenerf_amd import fused
    rng = np.random.default_rng(24)
    torch.manual_seed(24)
    mk = lambda: gridencoder.GridEncoder(input_dim=3, num_levels=6, level_dim=2, per_level_scale=2, base_resolution=8, log2_hashmap_size=10, gridtype=gridtype,
                                         align_corners=True).to(cuda)
    ea, eb = mk(), mk()
    for e in (ea, eb):
        e.embeddings.data.uniform_(-0.5, 0.5)
    assert fused.pairable(ea, eb)
    _, _, _, x = _grid_setup(rng, 6, 8, 10, None, 2, 3001)
    x01 = dev(x, cuda)
    a, b = fused.grid_encode_raw_pair(ea, eb, x01)
    for got, e in ((a, ea), (b, eb)):
        assert torch.equal(got, fused.grid_encode_raw(e, x01))
        want = oracle.grid_encode_forward(x, host(e.embeddings.detach()), host(e.offsets), 2.0, 8, gridtype=e.gridtype_id, align_corners=True, raw=True)
        np.testing.assert_array_equal(host(got), want)
    assert float(a[:, 3].abs().max()) == 0.0 and float(b[:, 4].abs().max()) == 0.0      # the two points outside [0, 1]^3


def test_grid_encode_align_corners_wraps_the_corner_beyond_a_dense_level(cuda):
    """align_corners: side == resolution, so an input of exactly 1.0 puts the +1 corner at index side on that axis and (z == 1.0) the row index at
    or beyond side^3 -- the reference wraps it with `% hashmap_size` (gridencoder.cu:49-72).  Its weight is 0, so a kernel that skips the wrap on
    dense levels gives the same numbers UNLESS the stray row (the next level's first rows) is not finite: those rows are NaN here."""
    rng = np.random.default_rng(23)
    L, H = 4, 8
    offsets = oracle.grid_offsets(3, L, 2.0, H, 19, align_corners=True)      # 8^3, 16^3, 32^3, 64^3 rows: all dense, sizes == side^3
    emb = (rng.random((int(offsets[-1]), 2)) - 0.5).astype(np.float32)
    x = np.minimum(0.5 + 0.5 * rng.random((4001, 3)), 0.999).astype(np.float32)   # coordinates in [0.5, 1): no genuine read of a level's first rows
    x[:64, 2] = 1.0     # corner z + 1 == side: index side^3 + x + y side -- wrapped: rows >= (side/2 - 1)(side + 1) of this level; not wrapped: the next level's first rows
    for lv in range(1, L):
        side = H << (lv - 1)                                           # resolution of the level BEFORE this one
        emb[offsets[lv]: offsets[lv] + side * side + side + 8] = np.nan
    want = oracle.grid_encode_forward(x, emb, offsets, 2.0, H, gridtype=0, align_corners=True)
    assert np.isfinite(want).all()
    out = gridencoder.grid_encode(dev(x, cuda), dev(emb, cuda), dev(offsets, cuda), 2.0, H, False, 0, True)
    np.testing.assert_array_equal(host(out), want)


def test_grid_encode_forward_fp16_table_bit_exact(cuda):
    rng = np.random.default_rng(21)
    pls, offsets, emb, x = _grid_setup(rng, 16, 16, 19, 4096, 2, 10007)
    emb16 = emb.astype(np.float16)
    out = gridencoder.grid_encode(dev(x, cuda), dev(emb16, cuda), dev(offsets, cuda), pls, 16, False, 0, False)
    assert out.dtype == torch.float16
    want = oracle.grid_encode_forward(x, emb16, offsets, pls, 16)
    np.testing.assert_array_equal(host(out).view(np.uint16), want.view(np.uint16))  # half accumulator reproduced bit for bit
    # autocast path of the reference (grid.py:38-39): fp32 parameter, half table on the fly
    with torch.autocast("cuda", dtype=torch.float16):
        out2 = gridencoder.grid_encode(dev(x, cuda), dev(emb, cuda), dev(offsets, cuda), pls, 16, False, 0, False)
    np.testing.assert_array_equal(host(out2).view(np.uint16), want.view(np.uint16))


def test_grid_forward_d3c2_kernel_and_row_layout_are_bit_identical(cuda):
    """k_grid_fwd_d3c2 (the D = 3, C = 2 lookup: addresses first, finest levels first, index by kind of level) against the generic kernel,
    and its [B, L*C] row output against the [L, B, C] one: same bits.  Covers dense levels, hashed levels of power-of-two size, a hashed level
    whose size is NOT a power of two (hand-made offsets: the reference's `%`), the tiled grid, align_corners, fp16 tables, and the oracle."""
    import ctypes
    from palettenerf_amd import _lib
    from palettenerf_amd._torch_glue import call, ptr
    lib = _lib.load()
    u32, f32, cint = ctypes.c_uint32, ctypes.c_float, ctypes.c_int
    rng = np.random.default_rng(77)
    cases = []
    pls, offsets, emb, x = _grid_setup(rng, 16, 16, 19, 4096, 2, 30011)
    cases.append(("shipped", pls, 16, offsets, emb, x, 0, False))
    pls, offsets, emb, x = _grid_setup(rng, 6, 8, 10, None, 2, 5003)
    cases += [("tiled", pls, 8, offsets, emb, x, 1, False), ("hash_ac", pls, 8, offsets, emb, x, 0, True), ("tiled_ac", pls, 8, offsets, emb, x, 1, True)]
    # odd level sizes: rows per level that are neither (res+1)^3 nor a power of two (the C ABI takes any offsets)
    sizes = np.array([1000, 3000, 5000, 7777, 10001, 4093], dtype=np.int64)
    offs_odd = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    emb_odd = (rng.random((int(offs_odd[-1]), 2)) - 0.5).astype(np.float32)
    cases.append(("odd_sizes", 2.0, 8, offs_odd, emb_odd, x, 0, False))
    try:
        for name, pls, H, offsets, emb, x, gridtype, ac in cases:
            L, B = len(offsets) - 1, x.shape[0]
            S = float(np.log2(pls))
            for dtype_id, tab in ((0, emb), (1, emb.astype(np.float16))):
                tx, tt, to = dev(x, cuda), dev(tab, cuda), dev(offsets, cuda)
                outs = {}
                for label, fast, layout in (("generic", 0, 0), ("fast_levels", 1, 0), ("fast_rows", 1, 1)):
                    assert lib.pnr_set_option(b"grid_fast", fast) == 0
                    out = torch.full((B * L * 2,), 7.0, device=cuda, dtype=tt.dtype)
                    call("pnr_grid_encode_forward_layout", ptr(tx), ptr(tt), ptr(to), ptr(out), u32(B), u32(3), u32(2), u32(L), f32(S), u32(H), None, u32(gridtype), cint(int(ac)),
                         cint(dtype_id), cint(layout))
                    o = host(out)
                    outs[label] = o.reshape(B, L, 2) if layout else o.reshape(L, B, 2).transpose(1, 0, 2)
                bits = np.uint32 if dtype_id == 0 else np.uint16
                np.testing.assert_array_equal(np.ascontiguousarray(outs["generic"]).view(bits), np.ascontiguousarray(outs["fast_levels"]).view(bits), err_msg=name)
                np.testing.assert_array_equal(np.ascontiguousarray(outs["generic"]).view(bits), np.ascontiguousarray(outs["fast_rows"]).view(bits), err_msg=name)
                want = oracle.grid_encode_forward(x, tab, offsets, pls, H, gridtype=gridtype, align_corners=ac)
                np.testing.assert_array_equal(np.ascontiguousarray(outs["fast_rows"]).reshape(B, L * 2).view(bits), want.view(bits), err_msg=name)
        # the generic kernel has no row layout: refused, not silently level-major
        assert lib.pnr_set_option(b"grid_fast", 0) == 0
        with pytest.raises(RuntimeError, match="unsupported"):
            call("pnr_grid_encode_forward_layout", ptr(tx), ptr(tt), ptr(to), ptr(out), u32(B), u32(3), u32(2), u32(L), f32(S), u32(H), None, u32(0), cint(0), cint(1), cint(1))
    finally:
        lib.pnr_set_option(b"grid_fast", 1)


def test_grid_encoder_module_against_the_reference_wrapper_fixture_fp32_and_autocast(cuda, golden_dir):
    """tests/golden/grid_autocast.npz was produced by the reference's own GridEncoder / _grid_encode (gridencoder/grid.py, imported in the
    build container over the CPU oracle): once in fp32, once with autocast on (the table goes to half, grid.py:36-39).  The product module under
    a real torch.autocast("cuda") must return the very same half bits; in fp32 the very same floats."""
    import os
    fx = np.load(os.path.join(golden_dir, "grid_autocast.npz"))
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096)
    assert np.array_equal(enc.offsets.numpy(), fx["offsets"]) and float(enc.per_level_scale) == float(fx["per_level_scale"])
    g = torch.Generator().manual_seed(int(fx["seed"]))
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=g) - 0.5))
    x = torch.rand(2048, 3, generator=g) * 4 - 2
    x[:4] = torch.tensor([[2.0, 2.0, 2.0], [-2.0, -2.0, -2.0], [2.0000005, 0.0, 0.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(x.numpy(), fx["x"])     # same generator stream as the fixture's
    enc = enc.to(cuda)
    with torch.no_grad():
        y32 = enc(x.to(cuda), bound=float(fx["bound"]))
        with torch.autocast("cuda", dtype=torch.float16):
            y16 = enc(x.to(cuda), bound=float(fx["bound"]))
    np.testing.assert_array_equal(host(y32), fx["y32"])
    assert y16.dtype == torch.float16
    np.testing.assert_array_equal(host(y16).view(np.uint16), fx["y16_bits"])


def test_grid_encode_backward_and_input_grad(cuda):
    rng = np.random.default_rng(22)
    pls, offsets, emb, x = _grid_setup(rng, 16, 16, 19, 4096, 2, 4099)
    te = dev(emb, cuda).requires_grad_(True)
    tx = dev(x, cuda).requires_grad_(True)
    out = gridencoder.grid_encode(tx, te, dev(offsets, cuda), pls, 16, True, 0, False)
    g = rng.standard_normal(out.shape).astype(np.float32)
    (out * dev(g, cuda)).sum().backward()
    oout, odydx = oracle.grid_encode_forward(x, emb, offsets, pls, 16, calc_grad_inputs=True)
    ogg, ogi = oracle.grid_encode_backward(g, x, emb.shape, offsets, pls, 16, dy_dx=odydx)
    np.testing.assert_array_equal(host(out), oout)
    np.testing.assert_allclose(host(te.grad), ogg, rtol=1e-5, atol=1e-5)  # atomics order differs from the oracle's loop order
    np.testing.assert_allclose(host(tx.grad), ogi, rtol=1e-5, atol=1e-3)  # |dy_dx| ~ scale ~ 4e3 at the finest level
    assert abs(float(te.grad.double().sum()) - float(ogg.astype(np.float64).sum())) < 1e-2  # checksum of the scatter


def test_grid_encode_backward_fp16(cuda):
    rng = np.random.default_rng(23)
    pls, offsets, emb, x = _grid_setup(rng, 8, 16, 14, None, 2, 2000)
    te = dev(emb.astype(np.float16), cuda).requires_grad_(True)
    out = gridencoder.grid_encode(dev(x, cuda), te, dev(offsets, cuda), pls, 16, False, 0, False)
    g = (rng.standard_normal(out.shape) * 0.01).astype(np.float16)
    (out * dev(g, cuda)).sum().backward()
    ogg = oracle.grid_encode_backward(g.astype(np.float32), x, emb.shape, offsets, pls, 16)
    np.testing.assert_allclose(host(te.grad).astype(np.float32), ogg, rtol=2e-2, atol=2e-3)  # packed-half atomics round every add


def test_grid_encoder_module_state_dict_names_and_errors(cuda):
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    sd = enc.state_dict()
    assert set(sd) == {"embeddings", "offsets"} and sd["embeddings"].shape == (6328848, 2) and sd["offsets"].dtype == torch.int32
    assert enc.output_dim == 32 and float(sd["embeddings"].abs().max()) <= 1e-4
    y = enc(torch.rand(7, 5, 3, device=cuda) * 4 - 2, bound=2)
    assert y.shape == (7, 5, 32)
    with pytest.raises(RuntimeError, match="unsupported"):
        gridencoder.grid_encode(torch.rand(4, 3, device=cuda), torch.rand(100, 3, device=cuda), torch.tensor([0, 50, 100], dtype=torch.int32, device=cuda), 2.0, 4)
    with pytest.raises(RuntimeError):
        gridencoder.grid_encode(torch.rand(4, 3), torch.rand(100, 2), torch.tensor([0, 50, 100], dtype=torch.int32), 2.0, 4)  # CPU tensors: no fallback


# ------------------------------------------------------------------------------------------ SH
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sh_encode_forward_and_grad(cuda, degree, golden_dir):
    rng = np.random.default_rng(30 + degree)
    x = rng.standard_normal((10007, 3)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    tx = dev(x, cuda).requires_grad_(True)
    y = shencoder.sh_encode(tx, degree, True)
    oy, od = oracle.sh_encode_forward(x, degree, True)
    np.testing.assert_allclose(host(y), oy, rtol=2e-6, atol=2e-6)  # fp32 Horner vs the oracle's fp64 closed form
    g = rng.standard_normal(oy.shape).astype(np.float32)
    (y * dev(g, cuda)).sum().backward()
    np.testing.assert_allclose(host(tx.grad), oracle.sh_encode_backward(g, degree, od), rtol=1e-4, atol=1e-4)
    if degree <= 5:  # the reference's own torch encoder
        gold = np.load(f"{golden_dir}/sh_torch.npz")
        np.testing.assert_allclose(host(shencoder.sh_encode(dev(gold["x"], cuda), degree, False)), gold[f"y{degree}"], atol=2e-6)


@pytest.mark.parametrize("degree,t,B", [(4, 15, 100003), (4, 15, 1), (1, 63, 255), (7, 15, 257), (3, 1, 4096), (5, 39, 513), (2, 60, 257), (6, 28, 513)])
def test_sh_encode_cat_is_the_concatenation(cuda, degree, t, B):
    """pnr_sh_encode_cat_forward == torch.cat([sh_encode(d), tail]) bit for bit (color_net's input, nerf/network.py:109-115); the tail's
    gradient is the column slice, directions get none."""
    g = torch.Generator().manual_seed(B + degree)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1).to(cuda)
    tail = torch.randn(B, t, generator=g).to(cuda).requires_grad_(True)
    enc = shencoder.SHEncoder(degree=degree)
    ref = torch.cat([enc(d), tail], dim=-1)
    out = shencoder.sh_encode_cat(enc, d, tail)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_sh_encode_cat")
    assert torch.equal(out, ref)
    w = torch.randn(B, degree * degree + t, generator=g).to(cuda)
    (g_out,) = torch.autograd.grad((out * w).sum(), tail)
    (g_ref,) = torch.autograd.grad((ref * w).sum(), tail)
    assert torch.equal(g_out, g_ref)
    # outside the fused form's reach: the plain composition (directions that want a gradient; too many columns)
    d2 = d.clone().requires_grad_(True)
    assert type(shencoder.sh_encode_cat(enc, d2, tail).grad_fn).__name__ == "CatBackward0"
    assert type(shencoder.sh_encode_cat(shencoder.SHEncoder(degree=8), d, tail).grad_fn).__name__ == "CatBackward0"


def test_sh_matches_reference_cuda_polynomials_off_sphere(cuda, golden_dir):
    import ctypes
    from palettenerf_amd._torch_glue import call, ptr
    gold = np.load(f"{golden_dir}/sh_cuda_expr.npz")
    x = dev(gold["points"].astype(np.float32), cuda)
    B = x.shape[0]
    y = torch.empty(B, 64, device=cuda)
    dydx = torch.empty(B, 3 * 64, device=cuda)
    call("pnr_sh_encode_forward", ptr(x), ptr(y), ctypes.c_uint32(B), ctypes.c_uint32(3), ctypes.c_uint32(8), ptr(dydx))
    np.testing.assert_allclose(host(y), gold["y"], rtol=1e-5, atol=2e-5)
    d = host(dydx).reshape(B, 3, 64)
    for axis, key in enumerate(("dx", "dy", "dz")):
        np.testing.assert_allclose(d[:, axis], gold[key], rtol=1e-5, atol=1e-4)
    assert shencoder.SHEncoder(degree=8).output_dim == 64
    with pytest.raises(AssertionError):
        shencoder.SHEncoder(degree=9)


# ------------------------------------------------------------------------------------------ HSV
def test_hsv_round_trip_and_parity(cuda):
    rng = np.random.default_rng(40)
    rgb = rng.random((100003, 3)).astype(np.float32)
    rgb[:4] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0]]
    rgb[4:2000] = rng.standard_normal((1996, 3)) * 0.5 + 0.3  # negative / >1 colours occur in the edit path
    hsv = palette_utils.rgb_to_hsv(dev(rgb, cuda))
    np.testing.assert_allclose(host(hsv), oracle.rgb_to_hsv(rgb), rtol=1e-5, atol=1e-3)
    back = palette_utils.hsv_to_rgb(hsv)
    np.testing.assert_allclose(host(back), oracle.hsv_to_rgb(host(hsv)), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(back)[2000:], rgb[2000:], atol=5e-6)  # round trip on in-gamut colours
    assert palette_utils.rgb_to_hsv(torch.rand(3, 4, 5, 3, device=cuda)).shape == (3, 4, 5, 3)


# ------------------------------------------------------------------------------------------ fused MFMA field
@pytest.mark.parametrize("precision", [0, 1])  # PNR_FIELD_FP32 (exact fmaf chains) / PNR_FIELD_F16X3 (split-fp16 matrix path)
def test_fused_nerf_field_matches_oracle_and_torch(cuda, precision):
    from palettenerf_amd import network
    from palettenerf_amd.fused import NeRFFieldFused
    rng = np.random.default_rng(50)
    m = network.NeRFNetwork(bound=2, cuda_ray=True)
    scene.seed_field_(m, 3)
    m = m.to(cuda).eval()
    m._fused = NeRFFieldFused(m)
    m._fused.precision = precision
    for B in (1, 31, 32, 33, 255, 256, 257, 5000, 70001):
        x = (rng.random((B, 3)).astype(np.float32) * 4 - 2)
        d = rng.standard_normal((B, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        tx, td = dev(x, cuda), dev(d, cuda)
        with torch.no_grad():
            m.fused_field = False
            s_ref, c_ref = m(tx, td)
            m.fused_field = True
            s, c = m(tx, td)
        # vs the unfused torch/rocBLAS evaluation of the same module
        np.testing.assert_allclose(host(s), host(s_ref), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(host(c), host(c_ref), rtol=0, atol=2e-6)
        if B <= 5000:  # vs the oracle (sequential-k fmaf chains; the MFMA kernel permutes k within each layer)
            enc = oracle.grid_encode_forward((x + 2) / 4, host(m.encoder.embeddings), host(m.encoder.offsets), m.encoder.per_level_scale, 16)
            w = [host(l.weight) for l in list(m.sigma_net) + list(m.color_net)]
            so, co = oracle.nerf_field_forward(enc, d, *w)
            np.testing.assert_allclose(host(s), so, rtol=2e-5, atol=1e-7)
            np.testing.assert_allclose(host(c), co, rtol=0, atol=2e-6)
    # weights changed in place -> the packed blob must be refreshed
    with torch.no_grad():
        m.color_net[2].weight.mul_(0.5)
        s2, c2 = m(tx, td)
        m.fused_field = False
        s3, c3 = m(tx, td)
    np.testing.assert_allclose(host(c2), host(c3), atol=2e-6)
    assert np.abs(host(c2) - host(c)).max() > 1e-3


def test_fused_nerf_field_f16x2_is_inside_the_colour_contract(cuda):
    """PNR_FIELD_F16X2 (opt-in: the colour layers with their activations rounded once to fp16 -- two MFMAs per product; sigma_net keeps the split
    form): against the oracle's fp32 field on seeded weights the colours stay within 5e-5 (north-star contract: 1e-4) and sigma is the split form's
    to 2e-5; it is NOT the fp32-class path for colours (the split form is held to 2e-6 above).  A frame rendered with it has exactly the split form's
    samples and alphas, and a PSNR above 85 dB against it."""
    from palettenerf_amd import network
    from palettenerf_amd.fused import NeRFFieldFused
    rng = np.random.default_rng(51)
    m = network.NeRFNetwork(bound=2, cuda_ray=True)
    scene.seed_field_(m, 3)
    m = m.to(cuda).eval()
    m._fused = NeRFFieldFused(m)
    m._fused.precision = 2
    assert m._fused.effective_precision() == 2
    B = 5000
    x = (rng.random((B, 3)).astype(np.float32) * 4 - 2)
    d = rng.standard_normal((B, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    with torch.no_grad():
        m.fused_field = True
        s, c = m(dev(x, cuda), dev(d, cuda))
    enc = oracle.grid_encode_forward((x + 2) / 4, host(m.encoder.embeddings), host(m.encoder.offsets), m.encoder.per_level_scale, 16)
    w = [host(l.weight) for l in list(m.sigma_net) + list(m.color_net)]
    so, co = oracle.nerf_field_forward(enc, d, *w)
    err_c = np.abs(host(c) - co).max()
    err_s = np.abs(host(s) / so - 1).max()
    assert 1e-7 < err_c < 5e-5 and err_s < 2e-5, (err_c, err_s)       # really the rounded form for colours, inside the contract; sigma as the split form
    # a frame: same march, same sample count, colours within the contract
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.count_rendered, m.density_scale = "native", True, 100.0
    H = W = 128
    ro, rd = scene.get_rays(torch.from_numpy(scene.lookat_pose())[None], scene.intrinsics_from_fov(H, W), H, W)
    kw = dict(perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4, bg_color=1)
    with torch.no_grad():
        fast = m.render(ro.to(cuda), rd.to(cuda), **kw)
        m._fused.precision = 1
        ref = m.render(ro.to(cuda), rd.to(cuda), **kw)
    assert int(fast["rendered"].sum()) == int(ref["rendered"].sum())
    assert torch.equal(fast["weights_sum"], ref["weights_sum"]) and torch.equal(torch.nan_to_num(fast["depth"]), torch.nan_to_num(ref["depth"]))   # densities untouched
    diff = (fast["image"] - ref["image"]).abs().max().item()
    assert diff < 1e-4, diff
    assert scene.psnr(fast["image"].cpu(), ref["image"].cpu()) > 85.0


@pytest.mark.parametrize("pred_clip", [False, True])
def test_fused_palette_field_matches_torch_module(cuda, pred_clip):
    """Fused PaletteNeRF field + colour-basis composite vs the unfused module + the torch statement of palette/renderer.py:470-500."""
    import torch.nn.functional as F
    from palettenerf_amd import network, renderer
    from palettenerf_amd.fused import PaletteFieldFused
    rng = np.random.default_rng(60)
    opt = renderer.default_opt(pred_clip=pred_clip)
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=3.0)
    scene.seed_field_(m, 5)
    m = m.to(cuda).eval()
    m.offsets_weight, m.view_dep_weight = 0.7, 1.3
    fused = PaletteFieldFused(m)
    nb = 4
    for B in (1, 33, 256, 383, 384, 385, 4097, 12289):   # around the 256- and 384-sample workgroup tiles of the 8- and 12-wave kernels
        x = dev(rng.random((B, 3)).astype(np.float32) * 4 - 2, cuda)
        d = rng.standard_normal((B, 3)).astype(np.float32)
        d = dev(d / np.linalg.norm(d, axis=1, keepdims=True), cuda)
        with torch.no_grad():
            sigma, clip_feat, omega, offsets_radiance, view_dep, diffuse = m(x, d)
            offsets, radiance = offsets_radiance[..., :-1].reshape(B, nb, 3), offsets_radiance[..., -1:].reshape(B, 1, 1)
            basis_color = m.basis_color[None].clamp(0, 1)
            final = F.softplus(radiance) * (basis_color + m.offsets_weight * offsets)
            basis_rgb = omega.reshape(B, nb, 1) * final
            rgbs = basis_rgb.sum(-2) + m.view_dep_weight * view_dep
            want_aux = torch.cat([diffuse + view_dep, view_dep, omega, basis_rgb.reshape(B, -1), (basis_color + offsets).reshape(B, -1), clip_feat], dim=1)
            s, c, aux = fused(x, d)
        used = 50 if pred_clip else 34       # without a clip head its 16 (all-zero) channels are not part of the packed row
        assert aux.shape == (B, 52 if pred_clip else 36)
        np.testing.assert_allclose(host(s), host(sigma) * 3.0, rtol=3e-5, atol=1e-7)
        np.testing.assert_allclose(host(c), host(rgbs), rtol=0, atol=5e-6)
        np.testing.assert_allclose(host(aux[:, :used]), host(want_aux)[:, :used], rtol=0, atol=5e-6)
        assert float(aux[:, used:].abs().sum()) == 0.0 and float(want_aux[:, used:].abs().sum()) == 0.0



@pytest.mark.parametrize("nb,clip_dim,pred_clip,precision", [(4, 16, False, 1), (4, 16, True, 1), (6, 16, False, 1), (8, 32, True, 1), (4, 16, False, 0), (3, 8, True, 0)])
def test_fused_palette_network_heads_match_the_torch_module(cuda, nb, clip_dim, pred_clip, precision):
    """PaletteFieldFused.network_forward (pnr_palette_edit.mode 3: the kernel's row = what PaletteNetwork.forward returns, no composite) against
    the torch module, output by output -- 4 bases on the 12-wave kernel, other shapes on the generic one, split-fp16 and exact fp32."""
    from palettenerf_amd import network, renderer
    from palettenerf_amd.fused import PaletteFieldFused
    rng = np.random.default_rng(62)
    opt = renderer.default_opt(pred_clip=pred_clip, num_basis=nb, clip_dim=clip_dim)
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=3.0)
    scene.seed_field_(m, 11 + nb)
    m = m.to(cuda).eval()
    fused = PaletteFieldFused(m)
    fused.precision = precision
    for B in (1, 33, 385, 4097):
        x = dev(rng.random((B, 3)).astype(np.float32) * 4 - 2, cuda)
        d = rng.standard_normal((B, 3)).astype(np.float32)
        d = dev(d / np.linalg.norm(d, axis=1, keepdims=True), cuda)
        with torch.no_grad():
            want = m(x, d)
            got = fused.network_forward(x, d)
        names = ("sigma", "clip_feat", "omega", "offsets_radiance", "view_dep", "diffuse")
        assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in want] == [(B,), (B, clip_dim), (B, nb), (B, 3 * nb + 1), (B, 3), (B, 3)]
        np.testing.assert_allclose(host(got[0]), host(want[0]), rtol=3e-5, atol=1e-7)          # sigma UNSCALED, as the reference's forward returns it
        for name, g_, w_ in list(zip(names, got, want))[1:]:
            np.testing.assert_allclose(host(g_), host(w_), rtol=0, atol=5e-6, err_msg=name)
        if not pred_clip:
            assert float(got[1].abs().sum()) == 0.0


def _palette_reference_rows(m, x, d, nb):
    """The torch statement of palette/renderer.py:470-500 (no edit): sigma, rgbs and the packed aux row of the unfused module."""
    import torch.nn.functional as F
    B = x.shape[0]
    sigma, clip_feat, omega, offsets_radiance, view_dep, diffuse = m(x, d)
    offsets, radiance = offsets_radiance[..., :-1].reshape(B, nb, 3), offsets_radiance[..., -1:].reshape(B, 1, 1)
    basis_color = m.basis_color[None].clamp(0, 1)
    final = F.softplus(radiance) * (basis_color + m.offsets_weight * offsets)
    basis_rgb = omega.reshape(B, nb, 1) * final
    rgbs = basis_rgb.sum(-2) + m.view_dep_weight * view_dep
    aux = torch.cat([diffuse + view_dep, view_dep, omega, basis_rgb.reshape(B, -1), (basis_color + offsets).reshape(B, -1), clip_feat], dim=1)
    return sigma, rgbs, aux


@pytest.mark.parametrize("nb,clip_dim,pred_clip,precision", [(6, 16, False, 1), (8, 16, True, 1), (10, 32, True, 1), (4, 16, True, 0), (8, 16, False, 0), (1, 16, False, 1)])
def test_fused_palette_field_more_bases_wider_clip_and_exact_fp32(cuda, nb, clip_dim, pred_clip, precision):
    """num_basis is the number of rows of the extracted palette (main_palette.py:141), not a constant: 1..10 bases (offsets_radiance_net then
    has up to 31 outputs: a second output tile), clip heads up to 32 wide, and the exact-fp32 matrix path of the same kernel."""
    from palettenerf_amd import network, renderer
    from palettenerf_amd.fused import PaletteFieldFused
    rng = np.random.default_rng(61)
    opt = renderer.default_opt(pred_clip=pred_clip, num_basis=nb, clip_dim=clip_dim)
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=3.0)
    scene.seed_field_(m, 7 + nb)
    m = m.to(cuda).eval()
    m.offsets_weight, m.view_dep_weight = 0.7, 1.3
    fused = PaletteFieldFused(m)
    fused.precision = precision
    for B in (33, 4097):
        x = dev(rng.random((B, 3)).astype(np.float32) * 4 - 2, cuda)
        d = rng.standard_normal((B, 3)).astype(np.float32)
        d = dev(d / np.linalg.norm(d, axis=1, keepdims=True), cuda)
        with torch.no_grad():
            sigma, rgbs, want_aux = _palette_reference_rows(m, x, d, nb)
            s, c, aux = fused(x, d)
        used = 6 + 7 * nb + (clip_dim if pred_clip else 0)
        assert aux.shape == (B, (used + 3) // 4 * 4) and fused.effective_precision() == precision
        np.testing.assert_allclose(host(s), host(sigma) * 3.0, rtol=3e-5, atol=1e-7)
        np.testing.assert_allclose(host(c), host(rgbs), rtol=0, atol=5e-6)
        np.testing.assert_allclose(host(aux[:, :used]), host(want_aux)[:, :used], rtol=0, atol=5e-6)
        assert float(aux[:, used:].abs().sum()) == 0.0
    with pytest.raises(RuntimeError):
        PaletteFieldFused(network.PaletteNetwork(renderer.default_opt(num_basis=11), bound=2, cuda_ray=True).to(cuda))


@pytest.mark.parametrize("model_kind", ["nerf", "palette"])
def test_split_fp16_field_with_tables_at_the_reference_init_scale(cuda, model_kind):
    """Hash tables as the reference initialises them, U(-1e-4, 1e-4) (gridencoder/grid.py:107): encoder features of ~1e-5, whose low fp16 halves
    would be subnormal.  The kernel prescales them by a power of two (enc_scale), so sigma_net's outputs keep fp32-class RELATIVE accuracy."""
    from palettenerf_amd import network, renderer
    from palettenerf_amd.fused import NeRFFieldFused, PaletteFieldFused, density_fused
    rng = np.random.default_rng(62)
    if model_kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True)
    else:
        m = network.PaletteNetwork(renderer.default_opt(pred_clip=True), bound=2, cuda_ray=True)
    scene.seed_field_(m, 9, table_range=1e-4)
    m = m.to(cuda).eval()
    B = 20000
    x = dev(rng.random((B, 3)).astype(np.float32) * 4 - 2, cuda)
    d = rng.standard_normal((B, 3)).astype(np.float32)
    d = dev(d / np.linalg.norm(d, axis=1, keepdims=True), cuda)
    with torch.no_grad():
        m.fused_field = False
        ref = m.density(x)
        m.fused_field = True
        got = m.density(x)                         # the fused density kernel (split-fp16)
    df = density_fused(m)
    assert df.effective_precision() == 1 and df.enc_scales()[0] == 8192.0
    g_ref, g_got = host(ref["geo_feat"]), host(got["geo_feat"])
    assert np.abs(g_ref).max() < 1e-3             # the features really are tiny
    assert np.abs(g_got - g_ref).max() <= 1e-5 * np.abs(g_ref).max()      # relative to the layer's scale: fp32-class (2e-4 without the prescale)
    np.testing.assert_allclose(host(got["sigma"]), host(ref["sigma"]), rtol=1e-6)
    with torch.no_grad():
        if model_kind == "nerf":
            m.fused_field = False
            s_ref, c_ref = m(x, d)
            m._fused = NeRFFieldFused(m)
            m.fused_field = True
            s, c = m(x, d)
            np.testing.assert_allclose(host(s), host(s_ref), rtol=1e-6)
            np.testing.assert_allclose(host(c), host(c_ref), atol=1e-6)
        else:
            fused = PaletteFieldFused(m)
            assert fused.enc_scales() == [8192.0, 8192.0, 8192.0]
            sigma, rgbs, want_aux = _palette_reference_rows(m, x, d, 4)
            s, c, aux = fused(x, d)
            np.testing.assert_allclose(host(s), host(sigma), rtol=1e-6)
            np.testing.assert_allclose(host(c), host(rgbs), atol=2e-6)
            np.testing.assert_allclose(host(aux[:, :50]), host(want_aux)[:, :50], atol=2e-6)
            clip_ref = host(want_aux[:, 34:50])
            assert np.abs(host(aux[:, 34:50]) - clip_ref).max() <= 1e-5 * np.abs(clip_ref).max()   # clip_net is prescaled too


@pytest.mark.parametrize("model_kind", ["nerf", "palette"])
@pytest.mark.parametrize("row_scale,overflows", [(4.0e4, True), (3.0e2, False), (4.0e6, None)])
def test_split_fp16_field_when_activations_can_leave_the_fp16_range(cuda, model_kind, row_scale, overflows):
    """One weight row scaled so that a hidden activation is huge.  fp16 holds magnitudes up to 65 504; beyond that a split operand is (inf, nan).
      * the static bound (largest table entry times the layers' L1 row norms) fails for both scales -> the stand-alone ops run exact fp32;
      * the device-driven loop keeps split-fp16 and WATCHES its operands: at 4e4 an activation really overflows -> the frame reports it, is
        rendered again in fp32 and the weights stay on fp32; at 3e2 nothing overflows (the bound is merely pessimistic) -> split-fp16 stays;
      * at 4e6 the WEIGHTS of that row are beyond fp16's range themselves (they are split into fp16 halves at pack time): exact fp32 at once.
    Frames in every mode agree with the torch loop."""
    import warnings
    from palettenerf_amd import network, renderer
    if model_kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    else:
        m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 11)
    with torch.no_grad():
        m.sigma_net[1].weight[1:].mul_(64.0)               # geometry features 64 x larger ...
        m.color_net[0].weight[:, 16:].mul_(1.0 / 64.0)     # ... which their consumers undo,
        if model_kind == "palette":
            m.diff_net[0].weight.mul_(1.0 / 64.0)
        m.color_net[0].weight[5, 16:].mul_(64.0)           # except hidden unit 5 of the view-dependent head,
        m.color_net[0].weight[5].mul_(row_scale)           # whose row is scaled up on top
        m.color_net[1].weight[:, 5].mul_(1.0 / row_scale)  # (its consumers scaled back so that the colours stay meaningful)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    ro, rd = rays_of(48, 48)
    ro, rd = dev(ro, cuda)[None], dev(rd, cuda)[None]
    kw = dict(perturb=False, dt_gamma=0.0, max_steps=1024, T_thresh=1e-4)
    if model_kind == "palette":
        kw["gui_mode"] = False
    out = {}
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for mode in ("compat", "fused", "native"):
            m.march_mode = "device" if mode == "fused" else mode
            m.fused_field = mode != "compat"
            if mode == "native":
                assert m._fused.frame_precision() == ((0, False) if overflows is None else (1, True))   # split-fp16 + watching, unless a weight is out of range
            out[mode] = m.render(ro, rd, **kw)
    assert m._fused.precision == 1 and m._fused.effective_precision() == 0            # stand-alone ops: the static bound sends them to fp32
    x = dev(np.random.default_rng(1).random((2304, 3)).astype(np.float32) * 1.2 - 0.6, cuda)
    with torch.no_grad():
        h = torch.relu(torch.cat([m.encoder_dir(rd[0]), m.density(x)["geo_feat"]], dim=-1) @ m.color_net[0].weight.t())
    if overflows is None:
        assert float(m.color_net[0].weight.abs().max()) > 65504.0 and m._fused.frame_precision() == (0, False) and not caught
    elif overflows:
        assert float(h.max()) > 65504.0 and float(m.color_net[0].weight.abs().max()) < 6.0e4   # the premise: only the ACTIVATION is too large for fp16
        assert m._fused.frame_precision() == (0, False)                               # latched after the frame reported the overflow
        assert any("fp16's range" in str(w.message) for w in caught)
    else:
        assert 100.0 < float(h.max()) < 65504.0
        assert m._fused.frame_precision() == (1, True) and not caught                 # nothing overflowed: split-fp16 stays, silently
    for mode in ("fused", "native"):
        for k in ("image", "weights_sum"):
            assert torch.isfinite(out[mode][k]).all()
            assert float((out[mode][k] - out["compat"][k]).abs().max()) < 1e-4, (mode, k)


def test_rgb_histogram_matches_oracle(cuda):
    rng = np.random.default_rng(70)
    rgb = (rng.random((200003, 3)) * 1.2 - 0.1).astype(np.float32)   # includes values below 0 and above 0.999 (clamped)
    w = rng.random(200003).astype(np.float32)
    for bpc in (1, 3, 5):
        bw, bc = palette_utils.compute_RGB_histogram(rgb, w, bpc)
        obw, obc = oracle.compute_RGB_histogram(rgb, w, bpc)
        assert bw.dtype == np.float64 and bc.dtype == np.float32 and bw.shape == (1 << (3 * bpc),) and bc.shape == (1 << (3 * bpc), 3)
        np.testing.assert_array_equal(bc, obc)
        np.testing.assert_allclose(bw, obw, rtol=1e-12)   # fp64 atomics: summation order differs from the serial loop
        assert abs(bw.sum() - w.astype(np.float64).sum()) < 1e-6
    bw, bc = palette_utils.compute_RGB_histogram(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), 2)
    assert bw.sum() == 0 and bc.shape == (64, 3)


def test_rgb_histogram_against_the_reference_build_and_hsv_through_its_binding(cuda, golden_dir):
    """pnr_rgb_histogram against the fixture the reference's own compiled compute_RGB_histogram produced (tests/golden/hist.npz), and -- when
    oracle/_ref holds the built module -- the reference's `_palette_func` pybind layer (palette/src/bindings.cpp, unmodified) driving this
    repo's HIP HSV kernels through the C ABI (csrc/shim/palette_func_hip.cpp): the drop-in at the native boundary.  The HSV half checks the
    BINDING (argument order, shapes, the in-place contract); no reference build of the HSV arithmetic exists (it is CUDA) -- that is pinned by
    the oracle and colorsys, not here."""
    g = np.load(f"{golden_dir}/hist.npz")
    for bpc in (1, 2, 3, 5):
        bw, bc = palette_utils.compute_RGB_histogram(g["colors_rgb"], g["weights"], bpc)
        np.testing.assert_array_equal(bc, g[f"bin_centers_{bpc}"])
        np.testing.assert_allclose(bw, g[f"bin_weights_{bpc}"], rtol=1e-13, atol=0)   # fp64 atomics: the order of the additions differs
    from oracle import ref_build
    if not ref_build.available():
        pytest.skip("oracle/_ref not built (it is built where /root/reference exists and travels with the snapshot)")
    mod = ref_build.load()
    rng = np.random.default_rng(71)
    rgb = rng.random((4099, 3)).astype(np.float32)
    t = dev(rgb, cuda)
    hsv = torch.empty_like(t)
    mod.rgb_to_hsv(rgb.shape[0], t, hsv)
    back = torch.empty_like(t)
    mod.hsv_to_rgb(rgb.shape[0], hsv, back)
    np.testing.assert_allclose(host(hsv), oracle.rgb_to_hsv(rgb), rtol=2e-6, atol=2e-4)
    np.testing.assert_allclose(host(back), rgb, atol=2e-6)
    assert torch.equal(hsv, palette_utils.rgb_to_hsv(t))                              # same kernel as the Python operator
    with pytest.raises(RuntimeError):
        mod.rgb_to_hsv(4, torch.zeros(4, 3), torch.zeros(4, 3))                        # CPU tensors are refused (TORCH_CHECK -> RuntimeError)


# ------------------------------------------------------------------------------------------ ray generation (f2)
def test_get_rays_bit_exact_vs_oracle_and_reference_golden(cuda, golden_dir):
    from palettenerf_amd import rays
    g = np.load(f"{golden_dir}/get_rays.npz")
    H, W = [int(v) for v in g["HW"]]
    poses = dev(g["poses"], cuda)
    ro, rd = rays.rays_from_indices(poses, g["intrinsics"], H, W)
    oo, od = oracle.get_rays(g["poses"], g["intrinsics"], H, W)
    np.testing.assert_array_equal(host(rd), od)                               # same scalar spec, correctly rounded sqrt / div on both sides
    np.testing.assert_array_equal(host(ro), oo)
    np.testing.assert_allclose(host(rd), g["full_d"], atol=1e-6, rtol=0)      # the reference's torch evaluation
    for key in ("rand", "patch", "pair", "err"):
        inds = dev(g[key + "_inds"], cuda)
        _, d = rays.rays_from_indices(poses, g["intrinsics"], H, W, inds)
        np.testing.assert_array_equal(host(d), oracle.get_rays(g["poses"], g["intrinsics"], H, W, g[key + "_inds"])[1])
        np.testing.assert_allclose(host(d), g[key + "_d"], atol=1e-6, rtol=0)
    # the drop-in surface: keys, shapes, index ranges of every sampling mode
    torch.manual_seed(3)
    for kw in (dict(N=-1), dict(N=128), dict(N=128, patch_size=4), dict(N=128, random_size=5), dict(N=128, error_map=torch.rand(2, 128 * 128))):
        r = rays.get_rays(poses, g["intrinsics"], H, W, **kw)
        n = H * W if kw["N"] < 0 else 128
        assert r["rays_o"].shape == (2, n, 3) and r["rays_d"].shape == (2, n, 3) and r["inds"].shape == (2, n)
        assert int(r["inds"].min()) >= 0 and int(r["inds"].max()) < H * W
        assert ("inds_coarse" in r) == ("error_map" in kw)
        np.testing.assert_allclose(host(r["rays_d"].norm(dim=-1)), 1.0, atol=1e-6)
    with pytest.raises(RuntimeError):
        rays.rays_from_indices(poses.double(), g["intrinsics"], H, W)


# ------------------------------------------------------------------------------------------ dense-layer weight gradient (training)
@pytest.mark.parametrize("n_in,n_out", [(32, 64), (64, 16), (31, 64), (64, 64), (64, 3), (15, 13), (35, 64), (1, 1)])
@pytest.mark.parametrize("dtypes", [(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.float32, torch.float16), (torch.float16, torch.float32)])
def test_linear_weight_grad_matches_float64(cuda, n_in, n_out, dtypes):
    from palettenerf_amd import linear
    g = torch.Generator().manual_seed(n_in * 100 + n_out)
    for B in (1, 2, 4097, 100003):
        x = torch.randn(B, n_in, generator=g).to(dtypes[0])
        dy = (torch.randn(B, n_out, generator=g) * 0.1).to(dtypes[1])
        ref = dy.double().t() @ x.double()                                      # exact products of the given (possibly fp16) values
        got = linear.weight_grad(x.to(cuda), dy.to(cuda))
        assert got.shape == (n_out, n_in) and got.dtype == torch.float32
        scale = float((dy.double().abs().t() @ x.double().abs()).max()) + 1e-30
        np.testing.assert_allclose(host(got), ref.numpy(), atol=4e-7 * scale, rtol=0)   # fp32 accumulation of B terms, pairwise-ish order
    # accumulate into an existing gradient, deterministic across calls
    out = torch.ones(n_out, n_in, device=cuda)
    linear.weight_grad(x.to(cuda), dy.to(cuda), out=out, accumulate=True)
    np.testing.assert_array_equal(host(out), host(got + 1.0))
    np.testing.assert_array_equal(host(linear.weight_grad(x.to(cuda), dy.to(cuda))), host(got))


def test_linear_module_gradients_match_nn_linear(cuda):
    from palettenerf_amd import linear
    torch.manual_seed(0)
    ours, theirs = linear.Linear(31, 64, bias=False).to(cuda), torch.nn.Linear(31, 64, bias=False).to(cuda)
    theirs.weight.data.copy_(ours.weight.data)
    x = torch.randn(50000, 31, device=cuda, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    w = torch.randn(50000, 64, device=cuda)
    (ours(x) * w).sum().backward()
    (theirs(x2) * w).sum().backward()
    np.testing.assert_allclose(host(ours.weight.grad), host(theirs.weight.grad), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(host(x.grad), host(x2.grad), rtol=1e-5, atol=1e-6)
    assert set(ours.state_dict()) == {"weight"}
    with torch.autocast("cuda", dtype=torch.float16):
        y = ours(x.detach())
    assert y.dtype == torch.float16
    y.float().sum().backward()                  # fp16 dY, fp32 X through the kernel
    with pytest.raises(RuntimeError):
        linear.weight_grad(torch.zeros(4, 65, device=cuda), torch.zeros(4, 3, device=cuda))


def test_linear_with_bias_gradients_match_float64(cuda):
    """The one dense layer with a bias (offsets_radiance_net, palette/network.py:111): weight and bias gradient through pnr_linear_wgrad /
    pnr_linear_bgrad against float64 sums; same state_dict entries as nn.Linear."""
    from palettenerf_amd import linear
    torch.manual_seed(1)
    lay = linear.Linear(15, 13).to(cuda)
    assert set(lay.state_dict()) == {"weight", "bias"}
    x = torch.randn(70001, 15, device=cuda, requires_grad=True)
    w = torch.randn(70001, 13, device=cuda)
    (lay(x) * w).sum().backward()
    xd, wd = x.detach().double().cpu(), w.double().cpu()
    np.testing.assert_allclose(host(lay.bias.grad), wd.sum(0).numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(host(lay.weight.grad), (wd.t() @ xd).numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(host(x.grad), (wd @ lay.weight.detach().double().cpu()).numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(linear.bias_grad(w.half())), w.half().double().cpu().sum(0).numpy(), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("case", ["hash16", "tiled", "small_table", "clustered"])
def test_grid_backward_binned_matches_oracle(cuda, case, monkeypatch):
    """The bucket-binned table gradient (csrc/grid_binned.hip) against the oracle's scatter loop and against the atomic kernel."""
    rng = np.random.default_rng(31)
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1)
    if case == "hash16":
        pls, offsets, emb, x = _grid_setup(rng, 16, 16, 19, 4096, 2, 70001)
        gridtype = 0
    elif case == "tiled":
        pls, offsets, emb, x = _grid_setup(rng, 8, 16, 15, None, 2, 9001)
        gridtype = 1
    elif case == "small_table":          # every level a single partial bucket
        pls, offsets, emb, x = _grid_setup(rng, 4, 4, 10, None, 2, 3000)
        gridtype = 0
    else:                                # all samples in one cell neighbourhood: one crowded bucket on the dense levels, split jobs
        pls, offsets, emb, x = _grid_setup(rng, 16, 16, 19, 4096, 2, 150000)
        x = (0.4 + 0.01 * rng.random(x.shape)).astype(np.float32)
        gridtype = 0
    L = len(offsets) - 1
    te = dev(emb, cuda).requires_grad_(True)
    out = gridencoder.grid_encode(dev(x, cuda), te, dev(offsets, cuda), pls, 16 if case != "small_table" else 4, False, gridtype, False)
    g = rng.standard_normal(out.shape).astype(np.float32)
    (out * dev(g, cuda)).sum().backward()
    binned = host(te.grad).copy()
    ogg = oracle.grid_encode_backward(g, x, emb.shape, offsets, pls, 16 if case != "small_table" else 4, gridtype=gridtype)
    scale = np.abs(ogg).max()
    # 'clustered': ~1e5 addends per table row; the oracle's sequential fp32 loop, the atomics and the LDS image each round in a
    # different order, so the tolerance there is the fp32 accumulation error of such sums (~1e-4 relative), not the kernel's
    rtol, atol = (5e-4, 5e-3) if case == "clustered" else (1e-5, 2e-6 * max(1.0, scale))
    np.testing.assert_allclose(binned, ogg, rtol=rtol, atol=atol)
    assert abs(float(binned.astype(np.float64).sum()) - float(ogg.astype(np.float64).sum())) < 1e-3 * max(1.0, float(np.abs(ogg).astype(np.float64).sum()) * 1e-4)
    # the coarsest levels as records (run-merged, split gather jobs) instead of LDS images: the round-1..3 path, still what a table with larger coarse levels takes
    from palettenerf_amd import _lib
    lib = _lib.load()
    try:
        for switch in (b"coarse_image", b"cell_merge"):      # ... and the mid levels without the merge of a cell's samples (a record per sample and corner)
            assert lib.pnr_set_option(switch, 0) == 0
            te.grad = None
            out = gridencoder.grid_encode(dev(x, cuda), te, dev(offsets, cuda), pls, 16 if case != "small_table" else 4, False, gridtype, False)
            (out * dev(g, cuda)).sum().backward()
            np.testing.assert_allclose(host(te.grad), ogg, rtol=rtol, atol=atol)
    finally:
        lib.pnr_set_option(b"coarse_image", 1)
        lib.pnr_set_option(b"cell_merge", 1)
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1 << 30)
    te.grad = None
    out = gridencoder.grid_encode(dev(x, cuda), te, dev(offsets, cuda), pls, 16 if case != "small_table" else 4, False, gridtype, False)
    (out * dev(g, cuda)).sum().backward()
    np.testing.assert_allclose(binned, host(te.grad), rtol=rtol, atol=atol)


@pytest.mark.parametrize("bound,H", [(1.0, 64), (4.0, 32), (2.0, 256), (1.0, 16)])
def test_march_other_grid_sizes_bit_exact(cuda, bound, H):
    """Occupancy grids other than 128^3 / two cascades: H = 64 (blocks of 16 cells still nest), H = 32 / 16 (block jumps off: H % 64 != 0;
    16 has no 4^3-brick mip words to spare), H = 256 (mip too large for LDS: plain path), one to three cascades."""
    C = 1 + int(np.ceil(np.log2(bound)))
    grid = scene.brick_density_grid(H=H, bound=bound, extent=0.65 * min(bound, 1.0))
    bf = scene.packbits_np(grid, 0.5)
    ro, rd = _far_rays(3000, 9)
    ro = ro * (bound / 8.0) * 2.0
    N = ro.shape[0]
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.05)
    for dt_gamma in (0.0, 1.0 / 128):
        cnt = np.zeros(2, np.int32)
        ox, od, odl, orays = oracle.march_rays_train(ro, rd, bound, bf, C, H, on, of, cnt, align=128, force_all_rays=True, dt_gamma=dt_gamma, max_steps=512)
        counter = torch.zeros(2, dtype=torch.int32, device=cuda)
        x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), bound, dev(bf, cuda), C, H, dev(on, cuda), dev(of, cuda), counter,
                                                      -1, False, 128, True, dt_gamma, 512)
        assert int(cnt[0]) > 1000
        np.testing.assert_array_equal(host(counter), cnt)
        np.testing.assert_array_equal(host(rays), orays)
        np.testing.assert_array_equal(host(x), ox)
        np.testing.assert_array_equal(host(dl), odl)


@pytest.mark.parametrize("max_steps", [1024, 16])
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
def test_march_sparse_scene_block_jumps_bit_exact(cuda, dt_gamma, max_steps):
    """Scene S1 (scattered 4^3 bricks, the occupied box ~94 % air): nearly every probe of a ray is an empty-block jump
    (csrc/march_core.hpp); counts, offsets, positions and deltas must still equal the oracle's cell-by-cell walk bit for bit.
    max_steps = 16 makes dt_min (2 sqrt3 / 16) LARGER than dt_max: clamp(x, dt_min, dt_max) = min(dt_max, max(dt_min, x)) then steps by dt_max,
    which is what the jumps' closed form has to use (round 3: it used dt_min there; the frame loops agreed with each other, not with this)."""
    grid = scene.sparse_density_grid()
    bf = scene.packbits_np(grid, 0.5)
    ro, rd = rays_of(96, 80)
    aabb = np.array([-2, -2, -2, 2, 2, 2], np.float32)
    on, of = oracle.near_far_from_aabb(ro, rd, aabb, 0.2)
    cnt = np.zeros(2, np.int32)
    ox, od, odl, orays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, on, of, cnt, align=128, force_all_rays=True, dt_gamma=dt_gamma, max_steps=max_steps)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    x, d, dl, rays = raymarching.march_rays_train(dev(ro, cuda), dev(rd, cuda), 2.0, dev(bf, cuda), 2, 128, dev(on, cuda), dev(of, cuda), counter,
                                                  -1, False, 128, True, dt_gamma, max_steps)
    assert int(cnt[0]) > (10000 if max_steps == 1024 else 1000)
    np.testing.assert_array_equal(host(counter), cnt)
    np.testing.assert_array_equal(host(rays), orays)
    np.testing.assert_array_equal(host(x), ox)
    np.testing.assert_array_equal(host(dl), odl)


@pytest.mark.parametrize("nb,n_in,frozen_h", [(4, 15, False), (5, 15, True), (1, 16, False), (10, 7, False)])
def test_palette_heads_match_the_torch_formulas(cuda, nb, n_in, frozen_h):
    """pnr_palette_heads_* against the reference's torch arithmetic for the two colour heads (palette/network.py:262-268: Linear with bias,
    Linear + Softplus, + 0.05, / row sum) evaluated in float64 with autograd: forward 2e-6, gradients 2e-5 of each tensor's largest
    gradient.  Rows around softplus' linear threshold, nb = 1 (omega == 1, zero gradient) and PNR_MAX_BASIS, a partial last tile."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(nb * 31 + n_in)
    M = 9000 + nb
    h = torch.randn(M, n_in, generator=g)
    w_or, b_or = torch.randn(3 * nb + 1, n_in, generator=g) * 0.3, torch.randn(3 * nb + 1, generator=g) * 0.1
    w_om = torch.randn(nb, n_in, generator=g) * 0.5
    h[:40] *= torch.linspace(5.0, 30.0, 40)[:, None]                 # pre-activations beyond F.softplus' threshold (20)
    w1, w2 = torch.randn(M, 3 * nb + 1, generator=g), torch.randn(M, nb, generator=g)

    def leafs(dtype, device):
        return [t.to(device=device, dtype=dtype).requires_grad_(not (frozen_h and k == 0)) for k, t in enumerate((h, w_or, b_or, w_om))]

    offrad, om, ref_grads, _ = f64.heads_block(h, w_or, b_or, w_om, w1, w2, torch.float64, "cpu", frozen_h)      # the reference arithmetic, float64 on the host

    h2, a2, b2, c2 = leafs(torch.float32, cuda)
    offrad2, om2 = palette_utils._palette_heads.apply(h2, a2, b2, c2)
    np.testing.assert_allclose(offrad2.detach().cpu().numpy(), offrad.numpy(), rtol=2e-6, atol=2e-5)
    np.testing.assert_allclose(om2.detach().cpu().numpy(), om.numpy(), rtol=2e-6, atol=2e-6)
    ((offrad2 * w1.to(cuda)).sum() + (om2 * w2.to(cuda)).sum()).backward()
    for name, got, want in zip(("h", "w_offsets_radiance", "b_offsets_radiance", "w_omega"), (h2, a2, b2, c2), ref_grads):
        if name == "h" and frozen_h:
            assert got.grad is None
            continue
        scale = float(want.abs().max()) + 1e-12
        err = float((got.grad.cpu().double() - want).abs().max())
        assert err <= 2e-5 * scale + 1e-7, (name, err, scale)


def test_palette_network_colour_heads_take_the_fused_kernel_in_training(cuda):
    """PaletteNetwork.color on a training batch routes the heads through pnr_palette_heads_* and gives the same outputs and parameter gradients
    as the layer-by-layer path (library GEMMs) to 1e-5 relative."""
    from palettenerf_amd import network, renderer, scene
    m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True)
    scene.seed_field_(m, 0)
    m = m.to(cuda).train()
    g = torch.Generator().manual_seed(3)
    M = 10000
    x = (torch.rand(M, 3, generator=g) * 2 - 1).to(cuda)
    d = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1).to(cuda)
    geo = torch.randn(M, 15, generator=g).to(cuda)
    wts = [torch.randn(M, k, generator=g).to(cuda) for k in (m.num_basis, 3 * m.num_basis + 1)]
    results = []
    for fused in (True, False):
        m.zero_grad(set_to_none=True)
        saved = network._fused_heads_ok
        if not fused:
            network._fused_heads_ok = lambda *_: False
        try:
            omega, offrad, _, _ = m.color(x, d, geo_feat=geo)
        finally:
            network._fused_heads_ok = saved
        ((omega * wts[0]).sum() + (offrad * wts[1]).sum()).backward()
        results.append((omega.detach(), offrad.detach(), m.offsets_radiance_net.weight.grad.clone(), m.offsets_radiance_net.bias.grad.clone(),
                        m.omega_net[0].weight.grad.clone(), m.encoder_palette.embeddings.grad.clone()))
    for a, b in zip(*results):
        scale = float(b.abs().max()) + 1e-12
        assert float((a - b).abs().max()) <= 1e-5 * scale + 1e-7


@pytest.mark.parametrize("nb,clip_dim,has_clip,has_smooth,frozen", [(4, 16, False, False, False), (4, 16, True, True, False), (6, 0, False, False, True),
                                                                    (1, 3, True, False, False), (16, 2, True, True, False)])
def test_palette_train_shade_matches_the_torch_formulas(cuda, nb, clip_dim, has_clip, has_smooth, frozen):
    """pnr_palette_train_shade_* against the reference's own torch arithmetic (palette/renderer.py:344-386) evaluated in float64 with autograd:
    forward 2e-6 relative, gradients 2e-5 relative to the largest gradient of each tensor.  Covers basis colours outside [0, 1] (clamp passes
    no gradient there), radiance beyond softplus' linear threshold, no clip head (zero columns), frozen basis colours, nb = 1 and 16."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(nb * 100 + clip_dim)
    M = 20000 + nb
    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale)
    omega = (F.softplus(rnd(M, nb)) + 0.05)
    omega = omega / omega.sum(-1, keepdim=True)
    offrad = rnd(M, 3 * nb + 1, scale=0.5)
    offrad[:50, -1] = torch.linspace(15.0, 30.0, 50)     # around F.softplus' threshold (20)
    view_dep, diffuse = torch.rand(M, 3, generator=g), torch.rand(M, 3, generator=g)
    clip_feat = rnd(M, clip_dim) if has_clip else None
    smooth = torch.rand(M, 1, generator=g) if has_smooth else None
    basis = torch.rand(nb, 3, generator=g) * 1.4 - 0.2   # some components outside [0, 1]
    w_rgb, w_all = rnd(M, 3), rnd(M, 13 + clip_dim + nb)

    def leafs(dtype, device):
        ts = [omega, offrad, view_dep, diffuse, clip_feat, smooth, basis]
        return [None if t is None else t.to(device=device, dtype=dtype).requires_grad_(True) for t in ts]

    # reference arithmetic, float64 on the host
    rgbs, all_ref, ref_grads = f64.shade_block(omega, offrad, view_dep, diffuse, clip_feat, smooth, basis, w_rgb, w_all, clip_dim, torch.float64, "cpu", frozen)

    o2, r2, vd2, df2, cf2, sm2, bc2 = leafs(torch.float32, cuda)
    rg, ab = palette_utils.palette_train_shade(o2, r2, vd2, df2, cf2, sm2, bc2.detach() if frozen else bc2, clip_dim)
    assert ab.shape == (M, 13 + clip_dim + nb)
    np.testing.assert_allclose(rg.detach().cpu().numpy(), rgbs.numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(ab.detach().cpu().numpy(), all_ref.numpy(), rtol=2e-6, atol=2e-6)
    ((rg * w_rgb.to(cuda)).sum() + (ab * w_all.to(cuda)).sum()).backward()
    for name, got, want in zip(f64.SHADE_NAMES, (o2, r2, vd2, df2, cf2, sm2, bc2), ref_grads):
        if got is None:
            continue
        if name == "basis_color" and frozen:
            assert got.grad is None
            continue
        scale = float(want.abs().max()) + 1e-12
        err = float((got.grad.cpu().double() - want).abs().max())
        assert err <= 2e-5 * scale + 1e-7, (name, err, scale)
    if not frozen:  # the clamp passes nothing where a basis colour lies outside [0, 1]
        outside = ((basis < 0) | (basis > 1))
        assert outside.any() and float(bc2.grad.cpu()[outside].abs().max()) == 0.0
    # deterministic: the basis-colour gradient is reduced in a fixed order
    if not frozen:
        first = bc2.grad.clone()
        bc2.grad = None
        rg, ab = palette_utils.palette_train_shade(o2, r2, vd2, df2, cf2, sm2, bc2, clip_dim)
        ((rg * w_rgb.to(cuda)).sum() + (ab * w_all.to(cuda)).sum()).backward()
        assert torch.equal(first, bc2.grad)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
@pytest.mark.parametrize("precision", [0, 1])
def test_fused_density_matches_the_torch_sigma_net(cuda, kind, precision):
    """pnr_nerf_density_forward (hash-grid lookup + sigma_net on the matrix cores) against the torch modules: sigma 2e-5 relative,
    geometry features 2e-5 absolute (fp32 GEMM order); both precision modes, both models, a batch that is not a multiple of the tile."""
    from palettenerf_amd import network, renderer
    from palettenerf_amd.fused import DensityFused
    if kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True)
    else:
        m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True)
    scene.seed_field_(m, 5)
    m = m.to(cuda).eval()
    g = torch.Generator().manual_seed(3)
    x = ((torch.rand(100003, 3, generator=g) * 2 - 1) * 2).to(cuda)
    with torch.no_grad():
        want = m.density(x)                      # fused_field is off: torch modules over the HIP encoder
    d = DensityFused(m)
    d.precision = precision
    sigma, geo = d(x)
    np.testing.assert_allclose(host(sigma), host(want["sigma"]), rtol=2e-5, atol=1e-30)
    np.testing.assert_allclose(host(geo), host(want["geo_feat"]), rtol=0, atol=2e-5)
    s2, none = d(x, scale=30.0, want_geo=False)
    assert none is None
    np.testing.assert_allclose(host(s2), host(sigma) * np.float32(30.0), rtol=1e-6)
    m.fused_field = True
    with torch.no_grad():
        got = m.density(x)                       # the module routes through the fused kernel now
    assert torch.equal(got["sigma"], d(x)[0]) or precision == 0


# One stack per instantiation the MLP's kernel tables (csrc/mlp.hip: g_mlp_fwd ... g_mlp_bwd_h) can be asked for through run_mlp: layers {2, 3} x input tiles of 32
# {1, 2} x output tiles {1, 2} x hidden activation {relu, elu}, every width odd or short of its tile somewhere.  Three layers with two tiles at both
# ends do not fit the backward's LDS (mlp.fusable refuses them; test_fused_mlp_widest_stack_forward_through_the_c_abi has their forward).
MLP_STACKS = [((20, 48, 9), "relu"), ((20, 48, 9), "elu"), ((9, 33, 50), "relu"), ((9, 33, 50), "elu"), ((40, 64, 17), "relu"), ((40, 64, 17), "elu"),
              ((40, 64, 33), "relu"), ((64, 50, 64), "elu"), ((24, 40, 64, 5), "relu"), ((24, 40, 64, 5), "elu"), ((16, 64, 32, 48), "relu"),
              ((30, 17, 64, 33), "elu"), ((33, 64, 64, 7), "relu"), ((33, 64, 64, 7), "elu")]
# ... of which the split-fp16 default lacked these
MLP_STACKS_SPLIT = [((20, 48, 9), "elu"), ((9, 33, 50), "relu"), ((40, 64, 33), "relu"), ((64, 50, 64), "elu"), ((24, 40, 64, 5), "elu"),
                    ((16, 64, 32, 48), "relu"), ((30, 17, 64, 33), "elu"), ((33, 64, 64, 7), "elu")]


@pytest.mark.parametrize("dims,act", [((31, 64, 64, 3), "relu"), ((15, 64, 64, 3), "relu"), ((35, 64, 15), "elu"), ((32, 64, 16), "relu"),
                                      ((7, 20, 40), "elu"), ((64, 33, 64, 16), "relu"),
                                      ((31, 64, 64, 3), "relu+sigmoid"), ((15, 64, 64, 3), "relu+sigmoid"), ((7, 20, 40), "elu+sigmoid")]
                         + MLP_STACKS_SPLIT + [(dims, act + "@fp32") for dims, act in MLP_STACKS])
def test_fused_mlp_forward_backward_match_float64(cuda, request, dims, act):
    """pnr_mlp_forward / pnr_mlp_backward (csrc/mlp.hip) against the layer loop in float64: output 2e-6 relative to the largest output,
    dX and every dW 2e-5 relative to that gradient's largest entry (fp32 accumulation over 5e4 samples).  Shapes of every net of both
    fields plus odd widths and a batch that is not a multiple of the 128-sample workgroup tile; dW is deterministic.
    "@fp32": the same with the exact fp32 launches ("mlp_f16x3" = 0), which the default never reaches."""
    import torch.nn.functional as F
    from palettenerf_amd import mlp, _lib
    act, _, arith = act.partition("@")
    if arith == "fp32":
        lib = _lib.load()
        request.addfinalizer(lambda: lib.pnr_set_option(b"mlp_f16x3", 1))
        assert lib.pnr_set_option(b"mlp_f16x3", 0) == 0
    torch.manual_seed(sum(dims))
    B = 50000 + 77
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(len(dims) - 1)]).to(cuda)
    for l in net:
        torch.nn.init.normal_(l.weight, std=1.0 / l.in_features ** 0.5)
    act, _, out_name = act.partition("+")
    out = torch.sigmoid if out_name == "sigmoid" else None     # the colour heads' torch.sigmoid inside the same launches (PNR_MLP_OUT_SIGMOID)
    fact = F.relu if act == "relu" else F.elu
    x = torch.randn(B, dims[0], device=cuda, requires_grad=True)
    wy = torch.randn(B, dims[-1], device=cuda)
    # a hidden unit whose pre-activation is within rounding of 0 may sit on either side of the kink in fp32 and float64: such samples
    # (a handful in 5e4 x 128 units) get no output gradient, so that the derivative choice cannot matter
    with torch.no_grad():
        ambiguous = f64.mlp_ambiguous(x, [l.weight for l in net], fact, "cpu", margin=2e-5)     # (the split-fp16 products are good to ~2^-22 of the largest term of a sum: a few 1e-6 on a pre-activation of order 1)
        assert int(ambiguous.sum()) < 2000
        wy[ambiguous.to(cuda)] = 0.0
    assert mlp.fusable(net, x, fact)
    y = mlp.run_mlp(net, x, fact, out)
    assert type(y.grad_fn).__name__.startswith("_FusedMLP")
    (y * wy).sum().backward()
    got = [x.grad.clone()] + [l.weight.grad.clone() for l in net]
    # float64 reference on the host
    h, want = f64.mlp_block(x, [l.weight for l in net], wy, fact, out, torch.float64, "cpu")
    scale = float(h.abs().max())
    assert float((y.detach().double().cpu() - h).abs().max()) <= 2e-6 * scale
    for name, a, b in zip(["dx"] + [f"dw{i}" for i in range(len(want) - 1)], got, want):
        err, ref = float((a.double().cpu() - b).abs().max()), float(b.abs().max())
        assert err <= 2e-5 * ref, (name, err, ref)
    for l in net:
        l.weight.grad = None
    x.grad = None
    (mlp.run_mlp(net, x, fact, out) * wy).sum().backward()
    assert all(torch.equal(l.weight.grad, g) for l, g in zip(net, got[1:]))
    # no input gradient wanted: same dW
    for l in net:
        l.weight.grad = None
    (mlp.run_mlp(net, x.detach(), fact, out) * wy).sum().backward()
    assert all(torch.equal(l.weight.grad, g) for l, g in zip(net, got[1:]))


@pytest.mark.parametrize("f16x3", [1, 0])
@pytest.mark.parametrize("dims,act", [((33, 64, 64, 40), "relu"), ((64, 50, 64, 64), "elu")])
def test_fused_mlp_widest_stack_forward_through_the_c_abi(cuda, dims, act, f16x3):
    """Three layers with more than 32 columns at both ends: pnr_mlp_forward takes them (k_mlp_fwd / k_mlp_fwd_h <3, 2, 2, .>), the backward has no LDS
    for them and palettenerf_amd.mlp never asks -- so the forward is called as a C caller would.  Against the float64 layer loop, to the forward bound of
    test_fused_mlp_forward_backward_match_float64; a batch of one 128-row workgroup tile and a bit."""
    import ctypes
    import torch.nn.functional as F
    from palettenerf_amd import mlp, _lib
    from palettenerf_amd._torch_glue import call, ptr
    lib = _lib.load()
    torch.manual_seed(sum(dims))
    B = 128 + 37
    ws = [torch.randn(dims[i + 1], dims[i], device=cuda) / dims[i] ** 0.5 for i in range(3)]
    fact = F.relu if act == "relu" else F.elu
    x = torch.randn(B, dims[0], device=cuda)
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(3)]).to(cuda)
    assert not mlp.fusable(net, torch.zeros(mlp.MIN_ROWS, dims[0], device=cuda, requires_grad=True), fact)
    desc = mlp._desc(list(dims), mlp._ACT[fact])
    packed = torch.empty(int(lib.pnr_mlp_packed_bytes(ctypes.byref(desc))) // 4, dtype=torch.float32, device=cuda)
    y = torch.empty(B, dims[-1], device=cuda)
    try:
        assert lib.pnr_set_option(b"mlp_f16x3", f16x3) == 0
        call("pnr_mlp_pack", ctypes.byref(desc), ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(packed))
        call("pnr_mlp_forward", ctypes.byref(desc), ptr(packed), ptr(x), ctypes.c_uint32(B), ptr(y))
        torch.cuda.synchronize()
    finally:
        lib.pnr_set_option(b"mlp_f16x3", 1)
    h, _ = f64.mlp_block(x, ws, torch.zeros(B, dims[-1]), fact, None, torch.float64, "cpu")
    scale = float(h.abs().max())
    err = float((y.double().cpu() - h).abs().max())
    assert scale > 0.1 and err <= 2e-6 * scale, (err, scale)


@pytest.mark.parametrize("dims,act,scale", [((32, 64, 64, 16), "relu", 1.0), ((35, 64, 15), "elu", 1.0), ((32, 64, 16), "relu", 1e-4), ((31, 64, 64, 3), "relu", 3e3)])
def test_fused_mlp_forward_split_fp16_against_the_exact_fp32_launch(cuda, dims, act, scale):
    """pnr_mlp_forward runs on the fp16 matrix pipe with split operands by default ("mlp_f16x3" = 1; csrc/mlp.hip): against the exact fp32 launch
    (option 0) within 2e-6 of the largest output, for inputs at the encoder's initialisation scale (1e-4: below fp16's normal range without the per-tile
    power-of-two scaling) and for large ones (3e3: products beyond fp16's range without it)."""
    import torch.nn.functional as F
    from palettenerf_amd import mlp, _lib
    lib = _lib.load()
    torch.manual_seed(11)
    B = 20000 + 5
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(len(dims) - 1)]).to(cuda)
    fact = F.relu if act == "relu" else F.elu
    x = torch.randn(B, dims[0], device=cuda) * scale
    x[:40] = 0.0                                        # an all-zero tile
    assert mlp.fusable(net, x, fact)
    try:
        assert lib.pnr_set_option(b"mlp_f16x3", 0) == 0
        want = mlp.run_mlp(net, x, fact, None).detach()
        assert lib.pnr_set_option(b"mlp_f16x3", 1) == 0
        got = mlp.run_mlp(net, x, fact, None)
        assert type(got.grad_fn).__name__.startswith("_FusedMLP")
        got = got.detach()
    finally:
        lib.pnr_set_option(b"mlp_f16x3", 1)
    ref = float(want.abs().max())
    assert ref > 0 and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 2e-6 * ref
    assert float(got[:32].abs().max()) == 0.0 or act == "elu"


@pytest.mark.parametrize("B", [1, 31, 33, 129, 4097])
def test_fused_mlp_split_fp16_on_small_and_ragged_batches(cuda, B, monkeypatch):
    """Both arithmetic forms of the fused MLP launches on batches smaller than a wave tile, one row past a tile, one workgroup and a bit: forward and
    every gradient of the split-fp16 launches against the exact fp32 ones (2e-6 / 2e-5 of the largest entry), an all-zero dY included."""
    import torch.nn.functional as F
    from palettenerf_amd import mlp, _lib
    lib = _lib.load()
    monkeypatch.setattr(mlp, "MIN_ROWS", 1)
    torch.manual_seed(B)
    dims = (32, 64, 64, 16)
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(3)]).to(cuda)
    x0 = torch.randn(B, dims[0], device=cuda)
    wy = torch.randn(B, dims[-1], device=cuda)
    res = {}
    try:
        for opt in (0, 1):
            assert lib.pnr_set_option(b"mlp_f16x3", opt) == 0
            x = x0.clone().requires_grad_(True)
            for l in net:
                l.weight.grad = None
            y = mlp.run_mlp(net, x, F.relu, None)
            assert type(y.grad_fn).__name__.startswith("_FusedMLP")
            (y * wy).sum().backward()
            res[opt] = [y.detach().clone(), x.grad.clone()] + [l.weight.grad.clone() for l in net]
        x = x0.clone().requires_grad_(True)
        (mlp.run_mlp(net, x, F.relu, None) * 0.0).sum().backward()           # dY == 0: every tile takes the "nothing to add" path
        assert float(x.grad.abs().max()) == 0.0
    finally:
        lib.pnr_set_option(b"mlp_f16x3", 1)
    for k, (a, b) in enumerate(zip(res[1], res[0])):
        ref = float(b.abs().max())
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= (2e-6 if k == 0 else 2e-5) * max(ref, 1e-30), (k, float((a - b).abs().max()), ref)


def test_grid_pair_lookup_is_bit_identical_to_two_lookups(cuda):
    """pnr_grid_encode_forward_pair (two tables of one geometry at the same points in one pass, rows interleaved) against two calls of the lookup op:
    bit for bit, out-of-range points included; the interleaved copy follows in-place updates of either table."""
    from palettenerf_amd import fused
    torch.manual_seed(2)
    ea = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    eb = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    ea.embeddings.data.uniform_(-0.5, 0.5)
    eb.embeddings.data.uniform_(-0.5, 0.5)
    assert fused.pairable(ea, eb)
    x01 = torch.rand(30011, 3, device=cuda)
    x01[7] = 1.5                                   # outside [0, 1]: zeros in both
    x01[8, 1] = -0.1
    for _ in range(2):
        a, b = fused.grid_encode_raw_pair(ea, eb, x01)
        assert torch.equal(a, fused.grid_encode_raw(ea, x01)) and torch.equal(b, fused.grid_encode_raw(eb, x01))
        assert float(a[:, 7].abs().max()) == 0.0 and float(b[:, 8].abs().max()) == 0.0
        with torch.no_grad():
            eb.embeddings.add_(0.25)               # an optimiser step: the pair table must be rebuilt


def test_grid_pair_copy_lives_on_the_encoder_and_notices_data_writes(cuda):
    """The training pair lookup's interleaved copy (fused._PairCopy): held by the first encoder (no global registry), dropped by
    invalidate_fused_caches, and a `.data` rewrite -- which moves neither identity nor version -- is noticed by the sampled checksum one call late."""
    import warnings
    from palettenerf_amd import fused

    class _M:                                     # what invalidate_fused_caches walks: a model's encoders
        pass
    torch.manual_seed(4)
    mk = lambda: gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    m = _M()
    m.encoder, m.encoder_palette = mk(), mk()
    for e in (m.encoder, m.encoder_palette):
        e.embeddings.data.uniform_(-0.5, 0.5)
    assert not hasattr(fused, "_PAIR_TABLES")
    x01 = torch.rand(5003, 3, device=cuda)
    same = lambda: all(torch.equal(p, fused.grid_encode_raw(e, x01)) for p, e in zip(fused.grid_encode_raw_pair(m.encoder, m.encoder_palette, x01), (m.encoder, m.encoder_palette)))
    assert same()
    assert "_pnr_pair" in m.encoder.__dict__ and "_pnr_pair" not in m.encoder.state_dict()
    # 1. a `.data` write followed by invalidate_fused_caches: fresh at once
    m.encoder.embeddings.data.uniform_(-0.25, 0.25)
    fused.invalidate_fused_caches(m)
    assert "_pnr_pair" not in m.encoder.__dict__
    assert same()
    # 2. a `.data` write nobody announces: stale for exactly one call, then noticed (warning) and rebuilt
    m.encoder_palette.embeddings.data.uniform_(-0.125, 0.125)
    assert not same()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert same()
    assert any("rewritten behind torch's version counters" in str(x.message) for x in w)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert same()
    assert not w
    # 2b. copy.deepcopy / pickling of an encoder that holds a copy (models are deep-copied by the optimiser tests and by users): the derived table (and the
    #     HIP event it carries) stays behind, the copy of the encoder builds its own
    import copy
    twin = copy.deepcopy(m.encoder)
    assert twin.__dict__.get("_pnr_pair") is None
    a2, _ = fused.grid_encode_raw_pair(twin, m.encoder_palette, x01)
    assert torch.equal(a2, fused.grid_encode_raw(m.encoder, x01))
    # 3. another partner: the copy is rebuilt for it
    other = mk()
    other.embeddings.data.uniform_(-0.5, 0.5)
    a, b = fused.grid_encode_raw_pair(m.encoder, other, x01)
    assert torch.equal(b, fused.grid_encode_raw(other, x01)) and torch.equal(a, fused.grid_encode_raw(m.encoder, x01))


@pytest.mark.parametrize("B", [1, 255, 257, 70001])
@pytest.mark.parametrize("degree,hw", [(1, 2), (3, 15), (4, 16), (6, 29), (7, 16)])
def test_sigma_geo_cat_matches_the_reference_composition(cuda, degree, hw, B):
    """shencoder.sigma_geo_cat -- trunc_exp(h[:, 0]) and cat([SH(d), h[:, 1:]]) as one launch each way (pnr_sigma_geo_cat_*) -- against the composition the
    reference writes (nerf/network.py:109-121 with activation.py's trunc_exp): forward bit for bit, the gradient of h to 1 ulp of exp (a logit beyond the
    clamp included).  Every SH degree's forward instantiation short of the 64-column limit or at it; h rows of 2 floats, of a power of two and of neither
    (the backward's block is the width rounded up to one); one row, a block less a row, a block and a row, many blocks."""
    from palettenerf_amd import shencoder as she
    from palettenerf_amd.activation import trunc_exp
    torch.manual_seed(3)
    enc = she.SHEncoder(degree=degree)
    h = torch.randn(B, hw, device=cuda)
    h[0, 0] = 20.0                                        # beyond the clamp of the gradient
    if B > 6:
        h[5, 0], h[6, 0] = 20.0, -20.0
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=cuda), dim=-1)
    w_s, w_c = torch.randn(B, device=cuda), torch.randn(B, degree * degree + hw - 1, device=cuda)
    h1 = h.clone().requires_grad_(True)
    s1, c1 = she.sigma_geo_cat(enc, h1, d)
    assert type(s1.grad_fn).__name__.startswith("_sigma_geo_cat")
    ((s1 * w_s).sum() + (c1 * w_c).sum()).backward()
    h2 = h.clone().requires_grad_(True)
    s2, c2 = trunc_exp(h2[..., 0]), torch.cat([enc(d), h2[..., 1:]], dim=-1)
    ((s2 * w_s).sum() + (c2 * w_c).sum()).backward()
    assert torch.equal(c1, c2)
    np.testing.assert_allclose(host(s1), host(s2), rtol=2e-7)
    np.testing.assert_allclose(host(h1.grad), host(h2.grad), rtol=3e-7, atol=0)
    # only one of the two outputs used
    h3 = h.clone().requires_grad_(True)
    s3, _ = she.sigma_geo_cat(enc, h3, d)
    (s3 * w_s).sum().backward()
    assert float(h3.grad[:, 1:].abs().max()) == 0.0
    np.testing.assert_allclose(host(h3.grad[:, 0]), host(h2.grad[:, 0]), rtol=3e-7)


@pytest.mark.parametrize("tail_w,dims,act", [(0, (32, 64, 16), "relu"), (3, (35, 64, 15), "elu"), (0, (32, 64, 64, 3), "relu")])
def test_encode_mlp_keeps_the_encoder_output_level_major(cuda, tail_w, dims, act):
    """mlp.encode_mlp (grid lookup -> [tail] -> MLP with the encoder output level-major end to end, pnr_mlp_*_lm + the binned table gradient)
    against the plain composition GridEncoder -> torch.cat -> layer loop: output 2e-6 of its scale, weight gradients 2e-5 and the table
    gradient 1e-4 of their largest entries (the table gradient sums ~1e5 addends per coarse row in a different order)."""
    import torch.nn.functional as F
    from palettenerf_amd import mlp
    torch.manual_seed(5 + tail_w)
    B = 40000 + 13
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    enc.embeddings.data.uniform_(-0.5, 0.5)
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(len(dims) - 1)]).to(cuda)
    fact = F.relu if act == "relu" else F.elu
    x = (torch.rand(B, 3, device=cuda) * 2 - 1) * 2
    tail = torch.rand(B, tail_w, device=cuda) if tail_w else None
    wy = torch.randn(B, dims[-1], device=cuda)
    y = mlp.encode_mlp(enc, x, 2, tail, net, fact)
    chain = [type(y.grad_fn).__name__] + [type(f[0]).__name__ for f in y.grad_fn.next_functions if f[0] is not None]
    assert any("EncodeMLP" in n for n in chain), chain      # the fused path ran
    (y * wy).sum().backward()
    got = [enc.embeddings.grad.clone()] + [l.weight.grad.clone() for l in net]
    enc.embeddings.grad = None
    for l in net:
        l.weight.grad = None
    mlp.enabled = False
    try:
        y2 = mlp.encode_mlp(enc, x, 2, tail, net, fact)      # plain composition (torch layer loop, library GEMMs)
        (y2 * wy).sum().backward()
    finally:
        mlp.enabled = True
    want = [enc.embeddings.grad] + [l.weight.grad for l in net]
    assert float((y - y2).abs().max()) <= 3e-6 * float(y2.abs().max())
    for name, a, b, tol in zip(["table"] + [f"dw{i}" for i in range(len(net))], got, want, [1e-4] + [3e-5] * len(net)):
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        assert err <= tol * ref, (name, err, ref)


def test_image_to_uint8_matches_the_host_conversion(cuda):
    """pnr_image_to_uint8 against what the reference does on the host before writing a frame, `(pred * 255).astype(np.uint8)`
    (nerf/utils.py:716-723): bit-exact, incl. exact 0 and 1, every byte boundary k/255 and its float neighbours, an odd element count and an
    unaligned view.  With linear_to_srgb (utils.py:43-44) the device powf may differ from torch's by an ulp: at most one level apart, < 0.01 %."""
    from palettenerf_amd import rays
    rng = np.random.default_rng(9)
    edges = np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.concatenate([rng.random(300001).astype(np.float32), [0.0, 1.0], edges, np.nextafter(edges, 2, dtype=np.float32), np.nextafter(edges, -1, dtype=np.float32).clip(0)])
    x = x.astype(np.float32)
    t = dev(x, cuda)
    got = host(rays.image_to_uint8(t))
    np.testing.assert_array_equal(got, (x * np.float32(255)).astype(np.uint8))
    view = t[1:-2]                                # not 16-byte aligned, odd length
    np.testing.assert_array_equal(host(rays.image_to_uint8(view)), (x[1:-2] * np.float32(255)).astype(np.uint8))
    img = t[:300000].reshape(100, 1000, 3)
    assert rays.image_to_uint8(img).shape == (100, 1000, 3)
    xt = torch.from_numpy(x)
    srgb = torch.where(xt < 0.0031308, 12.92 * xt, 1.055 * xt ** 0.41666 - 0.055).numpy()
    want = (srgb * np.float32(255)).astype(np.uint8)
    got = host(rays.image_to_uint8(t, linear_to_srgb=True))
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1 and (diff != 0).mean() < 1e-4


def test_palette_field_kernel_variants_are_bit_identical(cuda):
    """The 4-basis PaletteNeRF field has a specialised instantiation (no predication over the basis loops) that runs 12-wave workgroups; it
    must return the bits of the 8-wave one -- per-sample arithmetic does not depend on which lane, wave or tile a sample lands in -- and
    permuting the samples must permute the outputs.  (This is the test that exposed a VALU-write -> MFMA-read hazard behind the inline-asm
    fp16 split: results differed by 1e-6 from run to run until the wait states were added.)"""
    from palettenerf_amd import _lib, network, renderer
    from palettenerf_amd.fused import PaletteFieldFused
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=30.0, min_near=0.2)
    scene.seed_field_(m, 5)
    m = m.to(cuda).eval()
    f = PaletteFieldFused(m)
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    try:
        for B in (5000, 200000):
            x = (torch.rand(B, 3, generator=g) * 1.2 - 0.6).to(cuda)
            d = torch.randn(B, 3, generator=g)
            d = (d / d.norm(dim=1, keepdim=True)).to(cuda)
            perm = torch.randperm(B, generator=g).to(cuda)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(B, device=cuda)
            outs = []
            for w12 in (0, 1):
                assert lib.pnr_set_option(b"palette_waves12", w12) == 0
                for rep in range(3):     # run-to-run reproducibility too
                    outs.append(f(x, d))
                s, c, a = f(x[perm].contiguous(), d[perm].contiguous())
                outs.append((s[inv], c[inv], a[inv]))
            for o in outs[1:]:
                for u, v in zip(o, outs[0]):
                    assert torch.equal(u, v)
    finally:
        lib.pnr_set_option(b"palette_waves12", 1)


# ------------------------------------------------------------------------------------------ optimiser step
def test_fused_adam_is_bit_identical_to_torch_adam(cuda):
    """palettenerf_amd.optim.Adam (one launch for all tensors) against torch.optim.Adam with the reference's settings (main_palette.py:223):
    parameters AND both moment buffers must be the same bits after every step, for a table-sized tensor, small matrices, a tensor that gets
    no gradient, and sparse-looking gradients (mostly zeros, as the hash-table gradient is)."""
    from palettenerf_amd import _lib, optim
    g = torch.Generator(device="cpu").manual_seed(5)
    shapes = [(1 << 20, 2), (64, 32), (16, 64), (13, 15), (13,), (4, 3), (7,)]

    def make():
        gg = torch.Generator(device="cpu").manual_seed(6)
        return [torch.nn.Parameter(((torch.rand(s, generator=gg) - 0.5) * (1e-4 if i == 0 else 1.0)).to(cuda)) for i, s in enumerate(shapes)]

    grads = []
    for step in range(4):
        gs = []
        for i, s in enumerate(shapes):
            t = torch.randn(s, generator=g) * (10.0 ** (-step))
            if i == 0:
                t = t * (torch.rand(s, generator=g) < 0.05)     # 95 % exact zeros
            gs.append(None if (i == 6 or (i == 5 and step == 0)) else t.to(cuda))   # tensor 6 never trains; tensor 5 joins one step late
        grads.append(gs)

    def run(opt_cls, variant=None):
        ps = make()
        opt = opt_cls([{"params": ps[:3], "lr": 1e-2}, {"params": ps[3:], "lr": 1e-3}], betas=(0.9, 0.99), eps=1e-15)
        if variant is not None:
            assert _lib.load().pnr_set_option(b"adam_variant", variant) == 0
        out = []
        for gs in grads:
            for p, gr in zip(ps, gs):
                p.grad = None if gr is None else gr.clone()
            opt.step()
            out.append([p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps if len(opt.state[p]) for k in ("exp_avg", "exp_avg_sq")])
        return out, opt

    want, ref_opt = run(torch.optim.Adam)            # torch's default on the GPU: the foreach implementation
    matching = []
    for variant in range(8):
        got, my_opt = run(optim.Adam, variant)
        if all(torch.equal(a, b) for sa, sb in zip(got, want) for a, b in zip(sa, sb)):
            matching.append(variant)
    _lib.load().pnr_set_option(b"adam_variant", 0)
    assert 0 in matching, f"contraction variants that reproduce torch.optim.Adam bit for bit: {matching}"
    # same state layout: a torch.optim.Adam can continue from this optimiser's state_dict and vice versa
    sd = my_opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 4.0 and float(sd["state"][5]["step"]) == 3.0
    assert sd["state"].get(6, {}) == {}      # the tensor that never received a gradient has no optimiser state
    torch.optim.Adam(make_groups := [{"params": make()[:3]}, {"params": make()[3:]}], betas=(0.9, 0.99), eps=1e-15).load_state_dict(sd)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B,sig", [((3, 64, 15), 9001, False), ((35, 64, 3), 4097 + 13, True), ((15, 64, 64, 13), 8192 + 31, False), ((32, 64, 64, 16), 8192, False)])
def test_fused_mlp_tile_moves_on_odd_widths_and_ragged_ends(cuda, dims, B, sig, monkeypatch):
    """The fused MLP launches move their activation tiles as 16-byte requests (csrc/mlp.hip: raw_load / raw_to_stage / stage_to_global): a tile's 32 x width floats are
    one aligned run whatever the width, requests may straddle rows, and the launch's partial tile goes through rolled loops.  Widths that are not multiples of 4,
    batches that end inside a tile AND inside a 16-byte request (B x width not a multiple of 4), the sigmoid output, and an input view that starts off a 16-byte
    boundary (mlp.py copies it; the C entry refuses it): forward and every gradient against the torch layer loop."""
    import torch.nn.functional as F
    from palettenerf_amd import mlp, _lib
    monkeypatch.setattr(mlp, "MIN_ROWS", 1)
    torch.manual_seed(sum(dims) + B)
    n = len(dims) - 1
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(n)]).to(cuda)
    xfull = torch.randn(B + 1, dims[0], device=cuda)
    x_view = xfull[1:]                               # contiguous, but starts dims[0] * 4 bytes into the allocation
    out = torch.sigmoid if sig else None
    wy = torch.randn(B, dims[-1], device=cuda)

    def run(fused):
        x = x_view.detach().clone().requires_grad_(True) if not fused else x_view.detach().requires_grad_(True)
        for l in net:
            l.weight.grad = None
        if fused:
            y = mlp.run_mlp(net, x, F.relu, out)
            assert type(y.grad_fn).__name__.startswith("_FusedMLP")
        else:
            h = x
            for i, l in enumerate(net):
                h = l(h)
                if i != n - 1:
                    h = F.relu(h)
            y = torch.sigmoid(h) if sig else h
        (y * wy).sum().backward()
        return [y.detach(), x.grad] + [l.weight.grad.clone() for l in net]
    got, want = run(True), run(False)
    for k, (a, b) in enumerate(zip(got, want)):
        ref = float(b.abs().max())
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= (5e-6 if k == 0 else 5e-5) * max(ref, 1e-30), (k, float((a - b).abs().max()), ref)
    # the C entry itself refuses an array that starts off a 16-byte boundary
    if (x_view.data_ptr() % 16) != 0:
        lib = _lib.load()
        desc = _lib.MlpDesc()
        desc.n_layers = n
        for i, d in enumerate(dims):
            desc.dims[i] = d
        desc.activation = 0
        packed = torch.empty(int(lib.pnr_mlp_packed_bytes(ctypes.byref(desc))) // 4, dtype=torch.float32, device=cuda)
        y = torch.empty(B, dims[-1], device=cuda)
        rc = lib.pnr_mlp_forward(ctypes.byref(desc), packed.data_ptr(), x_view.data_ptr(), B, y.data_ptr(), None)
        assert rc == -4 and b"16-byte" in lib.pnr_error_string(rc)      # PNR_ERR_ALIGNMENT: the error says what is wrong


def test_fuse_field_palette_forward_follows_data_writes_to_the_tables(cuda):
    """dropin.fuse_field on a PaletteNetwork: torch_ema's copy_to / restore write the hash tables through `.data` (neither the version counter nor the storage
    moves).  The fused forward must read the tables as they are now -- within the tolerances of test_fused_palette_field_matches_torch_module against the
    module's own torch forward -- by default, and with the opt-in interleaved pair lookup after invalidate_fused_caches()."""
    from palettenerf_amd import dropin, network, renderer
    from palettenerf_amd.fused import invalidate_fused_caches
    rng = np.random.default_rng(63)
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=3.0)
    scene.seed_field_(m, 5)
    m = m.to(cuda).eval()
    dropin.fuse_field(m)
    B = 4097
    x = dev(rng.random((B, 3)).astype(np.float32) * 4 - 2, cuda)
    d = rng.standard_normal((B, 3)).astype(np.float32)
    d = dev(d / np.linalg.norm(d, axis=1, keepdims=True), cuda)

    def agree(got, what):
        with torch.no_grad():
            want = network.PaletteNetwork.forward(m, x, d)          # the module's own torch forward
        np.testing.assert_allclose(host(got[0]), host(want[0]), rtol=3e-5, atol=1e-7, err_msg=what)
        for g_, w_ in zip(got[1:], want[1:]):
            np.testing.assert_allclose(host(g_), host(w_), rtol=0, atol=5e-6, err_msg=what)

    with torch.no_grad():
        before = [t.clone() for t in m(x, d)]
    agree(before, "before the writes")
    keys = [(t._version, t.data_ptr()) for t in (m.encoder.embeddings, m.encoder_palette.embeddings)]
    other = (torch.rand(m.encoder.embeddings.shape, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(cuda)
    m.encoder.embeddings.data.copy_(other)
    m.encoder_palette.embeddings.data.mul_(-1)
    assert [(t._version, t.data_ptr()) for t in (m.encoder.embeddings, m.encoder_palette.embeddings)] == keys    # invisible to torch's counters
    with torch.no_grad():
        after = m(x, d)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[2], before[2])
    agree(after, "after the .data writes")
    m._fused.stand_alone_pair = True                                # the opt-in: the interleaved copy, which needs the explicit invalidation
    invalidate_fused_caches(m)
    with torch.no_grad():
        agree(m(x, d), "pair lookup after invalidate_fused_caches")
    m.encoder_palette.embeddings.data.mul_(-1)
    invalidate_fused_caches(m)
    with torch.no_grad():
        agree(m(x, d), "pair lookup, tables written back")


def test_flex_composite_after_a_fused_forward_outside_a_march_loop_is_written_on_return(cuda):
    """dropin.fuse_field arms the flex deferral behind every fused PaletteNetwork.forward under no_grad.  Outside run_cuda's loop (a point query, an export
    script) no march iteration is open: a direct composite_rays_flex that follows must have written its `output` when it returns -- as the same call with the
    deferral off.  The reference-style loop still reaches the device with one multi-map launch per iteration and no single flex launch."""
    from palettenerf_amd import _torch_glue, dropin, network, renderer
    rng = np.random.default_rng(92)
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=3.0, min_near=0.2)
    scene.seed_field_(m, 5)
    m = m.to(cuda).eval()
    dropin.fuse_field(m)
    x = dev(rng.random((512, 3)).astype(np.float32) * 2 - 1, cuda)
    d = torch.nn.functional.normalize(dev(rng.standard_normal((512, 3)).astype(np.float32), cuda), dim=-1)
    N, n_alive, n_step = 3000, 1700, 4
    alive = dev(np.sort(rng.choice(N, n_alive, replace=False)).astype(np.int32), cuda)
    M = n_alive * n_step
    sig, inp = dev((rng.random(M) * 60).astype(np.float32), cuda), dev(rng.standard_normal((M, 3)).astype(np.float32), cuda)
    dl = dev(np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32), cuda)
    t, ws = torch.rand(N, device=cuda), torch.rand(N, device=cuda) * 0.7
    try:
        with torch.no_grad():
            m(x, d)                                                 # a fused forward outside any march loop
        out = torch.zeros(N, 3, device=cuda)
        raymarching.composite_rays_flex(n_alive, n_step, 3, alive, t, sig, inp, dl, ws, out, 1e-4)
        got = out.clone()                                           # what the caller reads right on return
    finally:
        raymarching.flush_flex_composites()
    was = raymarching.defer_flex_composites(False)
    try:
        want = torch.zeros(N, 3, device=cuda)
        raymarching.composite_rays_flex(n_alive, n_step, 3, alive, t, sig, inp, dl, ws, want, 1e-4)
    finally:
        raymarching.defer_flex_composites(was)
    assert float(want.abs().sum()) > 0.0
    assert torch.equal(got, want)
    # the reference-style loop (the mirror's per-op loop with its seven flex composites per iteration)
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode = "compat"
    ro, rd = rays_of(32, 32)
    prof = _torch_glue.profile_kernels(["pnr_composite_rays", "pnr_composite_rays_flex", "pnr_composite_rays_flex_multi"])
    try:
        with torch.no_grad():
            r = m.render(dev(ro, cuda)[None], dev(rd, cuda)[None], dt_gamma=0.0, perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=False)
        torch.cuda.synchronize()
        n_comp, n_flex, n_multi = (len(prof[k]) for k in ("pnr_composite_rays", "pnr_composite_rays_flex", "pnr_composite_rays_flex_multi"))
    finally:
        _torch_glue.profile_kernels(None)
    assert float(r["weights_sum"].sum()) > 0.0
    assert n_comp > 1 and n_flex == 0 and n_multi == n_comp
