"""Jittered frames on the native frame loop (pnr_nerf_frame_args::noises, ABI 9) and the viewer step (pnr_present_frame, pipeline.viewer_frame /
ViewerAccumulator).

Fixtures: tests/golden/gen_golden_jitter.py -- the reference's own run_cuda(perturb=s) under torch.manual_seed(s), s in (2, 3), with the noise the
frame drew stored beside its maps: cases a / b of tests/test_gpu_frames.py and case c (case a's model marched with case b's dt_gamma = 1/128).
Tolerances are those of tests/test_gpu_frames.py for the same keys unjittered (COLOUR_TOL = DEPTH_TOL = 1e-4, the project's contract).  The
reference's jittered and unjittered frames, and its frames of the two seeds, differ on `image` by 1.1e-3 ... 3.6e-3 (a) and 1.7e-2 ... 4.2e-2 (c):
a frame that ignored the noise, or used the other seed's, fails here by 10x and more.  Case b's frames differ by 5.7e-4 ... 1.4e-3 only -- less than
the 10x the generator asks for, which it reports as an error at the end of its run; b is held to the same tolerances all the same."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from palettenerf_amd import network, pipeline, raymarching, renderer, scene
from palettenerf_amd import rays as prays

pytestmark = pytest.mark.gpu

COLOUR_TOL = 1e-4
DEPTH_TOL = 1e-4
# sRGB branch: the only operation that is not correctly rounded on both sides is powf (results in [0, 1]: a few ulp = a few times 6e-8, times 1.055).
# The pnr_image_to_uint8 test allows one level of 255 for it; on a float image that would let a wrong exponent or threshold through.
SRGB_TOL = 1e-6
NERF_KEYS = ["image", "depth", "weights_sum"]
GUI_KEYS = ["image", "depth", "depth_origin", "weights_sum", "clip_feat"]
FULL_KEYS = GUI_KEYS + ["direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"]
KW = dict(max_steps=1024, T_thresh=1e-4)


def load(golden_dir, kind, case):
    return np.load(os.path.join(golden_dir, f"frame_jitter_{kind}_{case}.npz"))


def make_model(kind, cuda, seed, density_scale, pred_clip=False):
    if kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2)
    else:
        m = network.PaletteNetwork(renderer.default_opt(pred_clip=pred_clip), bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2)
    scene.seed_field_(m, seed)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field, m.count_rendered = "native", True, True
    return m


def golden_model(kind, cuda, g):
    return make_model(kind, cuda, int(g["seed"]), float(g["density_scale"]), bool(g["pred_clip"]) if kind == "palette" else False)


def frame_rays(cuda, H, W, azimuth=45.0):
    pose = torch.from_numpy(scene.lookat_pose(azimuth_deg=azimuth))[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro.to(cuda), rd.to(cuda)


def gui(kind, on=True):
    return {"gui_mode": on} if kind == "palette" else {}


def close(got, want, tol, what):
    got = torch.as_tensor(got).detach().float().cpu().numpy().reshape(np.shape(want))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max abs err {err:.3g}")
    assert err <= tol, f"{what}: max abs err {err}"


def same(a, b, what="", min_maps=3):
    assert int(torch.as_tensor(a["rendered"]).sum()) == int(torch.as_tensor(b["rendered"]).sum()), what
    n = 0
    for k, v in a.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point and v.numel() > 1:
            assert torch.equal(torch.nan_to_num(v, nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (what, k)
            n += 1
    assert n >= min_maps, what


def tol_of(k):
    return DEPTH_TOL if k.startswith("depth") else COLOUR_TOL


# ---------------------------------------------------------------- 1. against the reference's jittered frames
@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_native_frame_with_stored_noises_matches_the_reference(cuda, golden_dir, kind, case):
    g = load(golden_dir, kind, case)
    m = golden_model(kind, cuda, g)
    ro, rd = frame_rays(cuda, int(g["H"]), int(g["W"]))
    keys = NERF_KEYS if kind == "nerf" else GUI_KEYS
    for s in (2, 3):
        noises = torch.from_numpy(g[f"noises_s{s}"]).to(cuda)
        with torch.no_grad():
            r = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), perturb=s, noises=noises, **gui(kind), **KW)
        assert "iterations" in r                      # the native loop's own key
        for k in keys:
            close(r[k], g[f"s{s}_{k}"], tol_of(k), f"{kind} {case} seed {s} {k}")
        other = g[f"s{5 - s}_image"]
        assert float(np.abs(r["image"].cpu().numpy().reshape(other.shape) - other).max()) > 2 * COLOUR_TOL     # not the other seed's frame
    if kind == "palette":
        with torch.no_grad():
            r = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), perturb=2, noises=torch.from_numpy(g["noises_s2"]).to(cuda), gui_mode=False, **KW)
        assert "iterations" in r
        for k in FULL_KEYS:
            close(r[k], g[f"full_s2_{k}"], tol_of(k), f"palette {case} full {k}")


# ---------------------------------------------------------------- 2. the same draw as the per-op loops
@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_perturb_under_one_seed_native_equals_the_per_op_loops(cuda, golden_dir, kind, case):
    g = load(golden_dir, kind, case)
    m = golden_model(kind, cuda, g)
    ro, rd = frame_rays(cuda, int(g["H"]), int(g["W"]))
    keys = NERF_KEYS if kind == "nerf" else GUI_KEYS
    out = {}
    for mode in ("native", "compat", "device"):
        m.march_mode, m.fused_field = mode, mode == "native"
        torch.manual_seed(11)
        with torch.no_grad():
            out[mode] = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), perturb=2, **gui(kind), **KW)
    assert "iterations" in out["native"] and "iterations" not in out["compat"]
    for mode in ("compat", "device"):
        assert int(out[mode]["rendered"].sum()) == int(out["native"]["rendered"].sum()), mode
        # (`rendered` = samples the march emitted, a frame total, as tests/test_gpu_frames.py compares the modes.  `n_samples` counts evaluated rows,
        # which the per-op march pads to a multiple of 128 per iteration: not comparable)
        for k in keys:
            close(out["native"][k], out[mode][k].cpu().numpy(), tol_of(k), f"{kind} {case} native vs {mode} {k}")


# ---------------------------------------------------------------- 3. zero noise, and the ray sort
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_zero_noise_is_the_plain_frame_and_noises_follow_the_ray_id(cuda, kind):
    from palettenerf_amd.fused import NeRFFieldFused, PaletteFieldFused, tile_ray_order
    m = make_model(kind, cuda, 5, 30.0)
    m._fused = (NeRFFieldFused if kind == "nerf" else PaletteFieldFused)(m)
    H, W = 40, 56
    ro, rd = frame_rays(cuda, H, W)
    kw = dict(dt_gamma=1.0 / 128, **gui(kind, False), **KW)
    noises = torch.rand(H * W, generator=torch.Generator().manual_seed(4)).to(cuda)
    with torch.no_grad():
        plain = m.render(ro, rd, perturb=False, **kw)
        zero = m.render(ro, rd, perturb=False, noises=torch.zeros(H * W, device=cuda), **kw)
        jit = m.render(ro, rd, perturb=False, noises=noises, **kw)
        m._fused.ray_order = tile_ray_order(torch.arange(H * W), W, 8).to(cuda)
        jit_tiles = m.render(ro, rd, perturb=False, noises=noises, **kw)
        m._fused.ray_order = torch.randperm(H * W, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(cuda)
        jit_perm = m.render(ro, rd, perturb=False, noises=noises, **kw)
        zero_perm = m.render(ro, rd, perturb=False, noises=torch.zeros(H * W, device=cuda), **kw)
    assert int(plain["rendered"].sum()) > 1000
    same(zero, plain, "zero noise")
    same(zero_perm, plain, "zero noise, permuted")
    assert float((jit["image"] - plain["image"]).abs().max()) > 2 * COLOUR_TOL
    same(jit_tiles, jit, "tile order")
    same(jit_perm, jit, "random order")
    with pytest.raises(RuntimeError, match="noises must be"):
        m.render(ro, rd, perturb=False, noises=noises[:-1], **kw)


# ---------------------------------------------------------------- 4. -O mode
@pytest.mark.parametrize("kind,pred_clip", [("nerf", False), ("palette", False), ("palette", True)])
def test_fp16_autocast_with_perturb_stays_on_the_native_loop(cuda, kind, pred_clip):
    m = make_model(kind, cuda, 7, 40.0, pred_clip)
    with torch.no_grad():
        for e in [m.encoder] + ([m.encoder_palette, m.encoder_clip] if kind == "palette" else []):
            e.embeddings.mul_(64.0)     # (tests/test_gpu_fp16_clip.py: with the tables as seeded half and fp32 lookups are ~1e-6 apart)
    ro, rd = frame_rays(cuda, 48, 40)
    kw = dict(dt_gamma=0.0, perturb=3, **gui(kind, False), **KW)
    torch.manual_seed(21)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = m.render(ro, rd, **kw)
    assert "iterations" in a and "grid_launches" in a and a["image"].dtype == torch.float32
    assert m._fused.table_half is False
    torch.manual_seed(21)
    with torch.no_grad():
        full = m.render(ro, rd, **kw)
        m._fused.table_half = True
        torch.manual_seed(21)
        b = m.render(ro, rd, **kw)
        m._fused.table_half = False
    same(a, b, "autocast vs explicit half tables")
    assert not torch.equal(torch.nan_to_num(a["image"]), torch.nan_to_num(full["image"]))       # the half tables were really used
    torch.manual_seed(21)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        plain = m.render(ro, rd, **(kw | {"perturb": False}))
    assert float((plain["image"] - a["image"]).abs().max()) > 2 * COLOUR_TOL                       # ... and so was the noise


# ---------------------------------------------------------------- 5. prepare / launch / finish
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_queue_frames_with_noises_equal_render(cuda, kind):
    m = make_model(kind, cuda, 0, 40.0)
    H, W = 96, 128
    intr = scene.intrinsics_from_fov(H, W)
    frames = []
    for i in range(5):      # poses 2 and 3 look past the object (few iterations): the frame behind them needs more than its submit call enqueues
        pose = scene.lookat_pose_from((3.0, 1.0, 0.5), target=(6.0, 2.5, 0.5)) if i in (2, 3) else scene.lookat_pose(azimuth_deg=20.0 + 61.0 * i, elevation_deg=25.0)
        ro, rd = scene.get_rays(torch.from_numpy(pose)[None], intr, H, W)
        frames.append((ro.to(cuda), rd.to(cuda)))
    noises = torch.rand(H * W, generator=torch.Generator().manual_seed(9)).to(cuda)
    kw = dict(dt_gamma=0, perturb=2, noises=noises, **gui(kind, False), **KW)
    with torch.no_grad():
        want = [m.render(ro, rd, **kw) for ro, rd in frames]
        plain = m.render(*frames[0], **(kw | {"noises": None, "perturb": False}))
    assert float((plain["image"] - want[0]["image"]).abs().max()) > 2 * COLOUR_TOL
    got = pipeline.render_queue(m, lambda i: frames[i], len(frames), **kw)
    for i, (a, b) in enumerate(zip(got, want)):
        assert "iterations" in a
        same(a, b, f"frame {i}")
    assert max(int(a["host_looks"]) for a in got) > 1          # a first chunk fell short: the finish call enqueued the rest, without a first iteration
    # perturb alone through the queue: the draw is made in render_prepare
    torch.manual_seed(5)
    with torch.no_grad():
        w = m.render(*frames[1], **(kw | {"noises": None}))
    torch.manual_seed(5)
    with torch.no_grad():
        q = m.render_finish(m.render_launch(m.render_prepare(*frames[1], **(kw | {"noises": None}))))
    same(q, w, "perturb through prepare / launch / finish")


# ---------------------------------------------------------------- 6. pnr_present_frame against torch
def torch_present(image, depth, rH, rW, H, W, ro=None, rd=None, depth_origin=None, clip_feat=None, srgb=False):
    """test_gui's expressions (palette/utils.py:1106-1119)."""
    def up(t):      # [1, rH, rW, C]
        if (rH, rW) == (H, W):
            return t
        return F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1).contiguous()
    out = {}
    preds = up(image.reshape(-1, rH, rW, 3).clamp(0, 1))
    if srgb:
        preds = torch.where(preds < 0.0031308, 12.92 * preds, 1.055 * preds ** 0.41666 - 0.055)
    out["image"] = preds[0]
    d = depth.reshape(-1, rH, rW)
    out["depth"] = (d if (rH, rW) == (H, W) else F.interpolate(d.unsqueeze(1), size=(H, W), mode="nearest").squeeze(1))[0]
    if depth_origin is not None:
        xyz = ro.reshape(-1, 3) + rd.reshape(-1, 3) * depth_origin.reshape(-1)[..., None]
        out["xyz"] = up(xyz.reshape(-1, rH, rW, 3))[0]
    if clip_feat is not None:
        out["clip_feat"] = up(clip_feat.reshape(-1, rH, rW, clip_feat.shape[-1]))[0]
    return out


@pytest.mark.parametrize("downscale", [1, 0.5, 0.37])
def test_present_frame_equals_the_torch_expressions(cuda, downscale):
    H, W = 45, 70
    rH, rW = int(H * downscale), int(W * downscale)
    n = rH * rW
    gen = torch.Generator().manual_seed(int(downscale * 100))
    rnd = lambda *shape: torch.rand(*shape, generator=gen).to(cuda)
    image = rnd(n, 3) * 1.4 - 0.2                 # values below 0 and above 1: the clamp works
    image[3, 1] = float("nan")
    depth, depth_origin = rnd(n), rnd(n) * 5
    ro, rd = rnd(n, 3) - 0.5, rnd(n, 3) - 0.5
    aux = rnd(n, 52)
    for clip in (aux[:, 34:50], aux[:, 32:48], aux[:, 3:8], rnd(n, 16), None):      # 8-byte rows, 16-byte rows, an odd width, contiguous, none
        for srgb in (False, True):
            got = pipeline.present_frame(image, depth, rH, rW, H, W, rays_o=ro, rays_d=rd, depth_origin=depth_origin, clip_feat=clip, linear_to_srgb=srgb)
            want = torch_present(image, depth, rH, rW, H, W, ro, rd, depth_origin, clip, srgb)
            assert set(got) == set(want)
            for k in want:
                assert got[k].shape == want[k].shape, k
                if k == "image" and srgb:
                    a, b = got[k], want[k]
                    assert torch.equal(torch.isnan(a), torch.isnan(b))
                    err = float((torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max())
                    print(f"downscale {downscale} sRGB image: max abs err {err:.3g}")
                    assert err <= SRGB_TOL
                else:
                    assert torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(want[k], nan=-7.0)), (k, downscale)
    # image and depth alone (a NeRF model's viewer frame), and the running mean of gui.py:225-231
    got = pipeline.present_frame(image, depth, rH, rW, H, W)
    want = torch_present(image, depth, rH, rW, H, W)
    assert set(got) == {"image", "depth"} and torch.equal(torch.nan_to_num(got["image"], nan=-7.0), torch.nan_to_num(want["image"], nan=-7.0))
    # (the mean is formed on HOST tensors, as the reference forms it on its numpy buffers: a true division.  On the device torch divides by a Python
    # scalar by multiplying with its reciprocal -- one ulp off for 3, 5, 6, 7 ... frames)
    accum = torch.full((H, W, 3), 123.0, device=cuda)
    buf = None
    for spp in range(5):
        img = rnd(n, 3) * 1.2
        out = torch_present(img, depth, rH, rW, H, W)["image"]
        buf = out.cpu() if spp == 0 else (buf * spp + out.cpu()) / (spp + 1)
        got = pipeline.present_frame(img, depth, rH, rW, H, W, accum=accum, accum_count=spp)
        assert torch.equal(got["image"], out) and torch.equal(accum.cpu(), buf), spp


# ---------------------------------------------------------------- 7. the viewer step
@pytest.mark.parametrize("kind,downscale", [("palette", 0.5), ("palette", 1), ("nerf", 0.37)])
def test_viewer_accumulator_equals_four_renders_averaged_in_torch(cuda, kind, downscale):
    m = make_model(kind, cuda, 3, 30.0, pred_clip=True)
    H, W = 60, 84
    rH, rW = int(H * downscale), int(W * downscale)
    pose = scene.lookat_pose(azimuth_deg=70.0)
    intr = scene.intrinsics_from_fov(H, W)
    acc = pipeline.ViewerAccumulator(m, W, H, max_spp=8)
    ro, rd = prays.rays_from_indices(torch.from_numpy(pose).float().reshape(1, 4, 4).to(cuda), [float(v) * downscale for v in intr], rH, rW, None)
    buf, spp, need_update = None, 1, True
    for k in range(4):
        torch.manual_seed(100 + k)
        got = acc.step(pose, intr, downscale=downscale, dt_gamma=0.0, **KW)
        assert "iterations" in got["frame"]
        torch.manual_seed(100 + k)
        with torch.no_grad():
            r = m.render(ro, rd, bg_color=None, perturb=False if spp == 1 else spp, dt_gamma=0.0, **gui(kind), **KW)
        pal = kind == "palette"
        want = torch_present(r["image"], r["depth"], rH, rW, H, W, ro if pal else None, rd if pal else None, r["depth_origin"] if pal else None,
                             r["clip_feat"] if pal else None)
        if need_update:       # (host tensors: the reference's buffers are numpy arrays, its mean a true division)
            buf, spp, need_update = want["image"].cpu(), 1, False
        else:
            buf, spp = (buf * spp + want["image"].cpu()) / (spp + 1), spp + 1
        assert set(want) <= set(got) and (("xyz" in got) == pal) and got["spp"] == spp
        for name, t in want.items():
            assert torch.equal(torch.nan_to_num(got[name], nan=-7.0), torch.nan_to_num(t, nan=-7.0)), (k, name)
        assert torch.equal(torch.nan_to_num(got["accum"].cpu(), nan=-7.0), torch.nan_to_num(buf, nan=-7.0)), k
    assert spp == 4 and float((buf - want["image"].cpu()).abs().max()) > 0           # frames 3 and 4 were jittered: the mean is not the last frame
    acc.reset()
    torch.manual_seed(1)
    got = acc.step(pose, intr, downscale=downscale, dt_gamma=0.0, **KW)
    assert got["spp"] == 1 and torch.equal(torch.nan_to_num(got["accum"]), torch.nan_to_num(got["image"]))
    acc.max_spp = 1
    assert acc.step(pose, intr, downscale=downscale, dt_gamma=0.0, **KW) is None
