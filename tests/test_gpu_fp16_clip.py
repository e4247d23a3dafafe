"""The native PaletteNeRF frame loop in the reference's -O mode with the clip head (main_palette.py ... -O --pred_clip --clip_dim 16): fp16 hash
tables through the interleaved half triple (k_frame_grid_h3, pnr_interleave_tables3_half), the field on its fp32-accurate path.

Fixtures: tests/golden/gen_golden_fp16_clip.py -- the reference's own run_cuda with forced-half lookups (`embeddings.to(torch.half)`, the three
encoder outputs upcast to fp32) and beside it the fp32-table frame, all three tables x64 (with the tables as seeded the two frames differ by
~1e-6 and no colour tolerance could tell them apart).

Tolerance (measured, not chosen): the existing native loop (fp32 triple) of the parent commit rendered the x64 fp32-table frames on an
MI355X against the x64 fp32 goldens; the largest error per map over both cases was
    image 3.8e-6, weights_sum 8.3e-7, clip_feat 5.1e-6, direct_rgb 7.7e-7, view_dep_rgb 5.1e-7, basis_rgb 3.1e-6, unscaled_basis_rgb 2.4e-6,
    basis_acc 3.7e-7, depth 6.3e-7, depth_origin 3.3e-6
(4 x the largest: 2.1e-5) and the bound is max(1e-4, 4 x measured) = 1e-4 for every map (GRAD_REL_TOL's rule in test_gpu_frames.py).  The reference's half and fp32
frames differ by 6.1e-3 / 1.5e-3 (image, case a / b) and 3.6e-3 / 5.3e-3 (clip_feat): more than 10x the bound (the generator asserts it)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from palettenerf_amd import network, raymarching, renderer, scene

pytestmark = pytest.mark.gpu

TOL = 1e-4
MAPS = ["image", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc", "depth", "depth_origin"]
KW = dict(perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=False)


def load(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"frame_palette_fp16_clip_{case}.npz"))


def clip_model(cuda, seed, density_scale, scale, grid=None):
    """A pred_clip PaletteNeRF mirror, its three hash tables multiplied by `scale` after seeding (as the generator does), on the brick scene."""
    m = network.PaletteNetwork(renderer.default_opt(pred_clip=True), bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2)
    scene.seed_field_(m, seed)
    with torch.no_grad():
        for e in (m.encoder, m.encoder_palette, m.encoder_clip):
            e.embeddings.mul_(scale)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid() if grid is None else grid).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field, m.count_rendered = "native", True, True
    return m


def rays(cuda, H, W, azimuth=45.0):
    pose = torch.from_numpy(scene.lookat_pose(azimuth_deg=azimuth))[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro.to(cuda), rd.to(cuda)


def half_frame(m, ro, rd, **kw):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return m.render(ro, rd, **(KW | kw))


def same(a, b, what=""):
    assert int(a["rendered"].sum()) == int(b["rendered"].sum()), what
    n = 0
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point and v.numel() > 1:
            assert torch.equal(torch.nan_to_num(v, nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (what, k)
            n += 1
    assert n >= len(MAPS), what


@pytest.mark.parametrize("case", ["a", "b"])
def test_clip_frame_under_fp16_autocast_takes_the_native_loop(cuda, golden_dir, case):
    g = load(golden_dir, case)
    m = clip_model(cuda, int(g["seed"]), float(g["density_scale"]), float(g["scale"]))
    ro, rd = rays(cuda, int(g["H"]), int(g["W"]))
    r = half_frame(m, ro, rd, dt_gamma=float(g["dt_gamma"]))
    assert "grid_launches" in r and "iterations" in r          # only the native loop sets them
    assert m._fused.table_half is False                        # restored
    assert r["image"].dtype == torch.float32
    for k in MAPS:
        got = r[k].detach().cpu().numpy()
        want = g[f"half_{k}"]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), k
        err = float(np.abs(got[fin] - want[fin]).max())
        print(f"case {case} {k}: max abs err {err:.3g} against the reference's half frame, "
              f"{float(np.abs(got[fin] - g[f'fp32_{k}'][fin]).max()):.3g} against its fp32 frame")
        assert err <= TOL, f"{k}: max abs err {err}"


@pytest.mark.parametrize("case", ["a", "b"])
def test_autocast_equals_explicit_half_tables(cuda, golden_dir, case):
    g = load(golden_dir, case)
    m = clip_model(cuda, int(g["seed"]), float(g["density_scale"]), float(g["scale"]))
    ro, rd = rays(cuda, int(g["H"]), int(g["W"]))
    a = half_frame(m, ro, rd, dt_gamma=float(g["dt_gamma"]))
    m._fused.table_half = True
    with torch.no_grad():
        b = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), **KW)
    assert int(a["rendered"].sum()) > 200
    same(a, b)


def test_queue_under_autocast_equals_render(cuda):
    m = clip_model(cuda, 7, 40.0, 64.0)
    frames = [rays(cuda, 64, 80, azimuth=az) for az in (20.0, 81.0, 142.0)]
    want = [half_frame(m, ro, rd, dt_gamma=0.0) for ro, rd in frames]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        pend = m.render_launch(m.render_prepare(*frames[0], dt_gamma=0.0, **KW))
        got = []
        for i in range(len(frames)):
            nxt = m.render_prepare(*frames[i + 1], dt_gamma=0.0, **KW) if i + 1 < len(frames) else None
            assert m.render_wait(pend)
            got.append(m.render_result(pend))
            if nxt is not None:
                pend = m.render_launch(nxt)
    assert m._fused.table_half is False
    for i, (a, b) in enumerate(zip(got, want)):
        assert "grid_launches" in a
        same(a, b, f"frame {i}")


@pytest.mark.parametrize("dt_gamma,density_scale,scene_kind", [(0.0, 1.0, "bricks"), (1.0 / 128, 0.02, "sparse"), (0.0, 0.05, "sparse")])
def test_hosted_march_tail_is_bit_identical_for_the_half_triple(cuda, dt_gamma, density_scale, scene_kind):
    """test_hosted_march_tail_is_bit_identical's matrix for the fp16 triple (k_frame_grid_h3 and its hosted tail)."""
    from palettenerf_amd import _lib
    from palettenerf_amd.fused import PaletteFieldFused
    lib = _lib.load()
    grid = scene.brick_density_grid() if scene_kind == "bricks" else scene.sparse_density_grid()
    m = clip_model(cuda, 3, density_scale, 1.0, grid=grid)
    m._fused = PaletteFieldFused(m)
    m._fused.table_half = True
    ro, rd = rays(cuda, 160, 200, azimuth=70.0)
    keys = ["image", "depth", "weights_sum", "rendered", "iterations", "view_dep_rgb", "diffuse_rgb", "direct_rgb", "basis_acc", "clip_feat", "omega_sparsity"]
    out = []
    try:
        for hosted, budget, budget0 in ((0, 2, 0), (1, 2, 0), (1, 1, 0), (1, 5, 3), (1, 1, 1)):
            assert lib.pnr_set_option(b"hosted_tail", hosted) == 0
            assert lib.pnr_set_option(b"march_budget", budget) == 0 and lib.pnr_set_option(b"march_budget0", budget0) == 0
            with torch.no_grad():
                r = m.render(ro, rd, perturb=False, dt_gamma=dt_gamma, max_steps=1024, T_thresh=1e-4)
            out.append({k: torch.as_tensor(r[k]).clone() for k in keys if k in r})
    finally:
        lib.pnr_set_option(b"hosted_tail", 1); lib.pnr_set_option(b"march_budget", 2); lib.pnr_set_option(b"march_budget0", 0)
    a = out[0]
    assert int(a["rendered"]) > 1000 and "clip_feat" in a
    for b in out[1:]:
        assert int(a["rendered"]) == int(b["rendered"])
        for k in a:
            assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), k


def test_interleave_tables3_half_equals_torch_half_casts(cuda):
    from palettenerf_amd import _lib
    lib = _lib.load()
    rows = 1000 + 3
    gen = torch.Generator().manual_seed(5)
    ts = [(torch.rand(rows, 2, generator=gen) - 0.5) * s for s in (2.0, 300.0, 1e5)]
    special = torch.tensor([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], [65504.0, 65519.0], [65520.0, -1e6], [6e-8, -3e-6], [2.0 ** -25, 1e-9],
                            [-0.0, 0.0], [float("inf"), float("-inf")], [1e-5 + 1e-9, 0.1]])
    for k, t in enumerate(ts):
        t[k * 8:(k + 1) * 8] = special.roll(k, 0)
    ts = [t.to(cuda).contiguous() for t in ts]
    out = torch.full((rows, 8), float("nan"), dtype=torch.float16, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.pnr_interleave_tables3_half(*[ctypes.c_void_p(t.data_ptr()) for t in ts], ctypes.c_uint64(rows), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s)) == 0
    want = torch.cat([t.to(torch.float16) for t in ts] + [torch.zeros(rows, 2, dtype=torch.float16, device=cuda)], dim=1)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.isinf(want).any() and (want.abs() < 6.1e-5).logical_and(want != 0).any()     # the inputs did reach inf and the subnormals


def test_half_triple_follows_table_updates(cuda):
    ro, rd = rays(cuda, 48, 40)
    m = clip_model(cuda, 11, 30.0, 64.0)

    def fresh(*edits):
        f = clip_model(cuda, 11, 30.0, 64.0)
        with torch.no_grad():
            for e in edits:
                e(f)
        return half_frame(f, ro, rd, dt_gamma=0.0)

    half_in_place = lambda x: x.encoder_clip.embeddings.mul_(0.5)
    flip = lambda x: x.encoder_clip.embeddings.data.copy_(x.encoder_clip.embeddings.data.flip(0))
    r0 = half_frame(m, ro, rd, dt_gamma=0.0)
    with torch.no_grad():
        half_in_place(m)
    r1 = half_frame(m, ro, rd, dt_gamma=0.0)
    assert not torch.equal(r1["clip_feat"], r0["clip_feat"])
    same(r1, fresh(half_in_place), "after mul_")
    flip(m)                                                    # a .data write: no version bump, the per-frame checksum notices
    with pytest.warns(UserWarning, match="rewritten behind torch's version counters"):
        r2 = half_frame(m, ro, rd, dt_gamma=0.0)
    assert not torch.equal(r2["clip_feat"], r1["clip_feat"])
    same(r2, fresh(half_in_place, flip), "after a .data write")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        same(half_frame(m, ro, rd, dt_gamma=0.0), r2, "again")
