"""The native frame loop off its power-of-two path: a bound that is no power of two (1.5; 3 with three cascades) and frames without an
occupancy mip.  make_frame_plan (csrc/frame.hip) picks k_frame_march<MIP, POW2, 1> from those two facts, the lookup kernels take the
division branch of unit_cube_of (csrc/grid_xside.hpp) and the hosted march tail is off -- every case asserts which instantiation it ran.

The reference is the host-driven mirror (march_mode "compat", no fused field) on the same model, as in
test_gpu_frames.py::test_native_loop_edge_cases_match_reference_style_loop: its per-op kernels are held bit for bit to the oracle at bound 1.5
(test_gpu_ops.py::test_march_rays_train_bit_exact, test_march_rays_inference_bit_exact).  Tolerances are that test's."""
import functools
import re

import pytest
import torch

from palettenerf_amd import _lib, network, raymarching, renderer, scene
from tests.test_gpu_frames import DEPTH_TOL, close

pytestmark = pytest.mark.gpu

TOL = 1e-4      # test_native_loop_edge_cases_match_reference_style_loop's own

# (bound, raymarching.USE_MIP) -> the (MIP, POW2, MODE) of the k_frame_march the frame has to launch
CONFIGS = {
    "bound1.5-mip": (1.5, True, (True, False, 1)),
    "bound3-mip": (3.0, True, (True, False, 1)),       # three cascades
    "bound2-nomip": (2.0, False, (False, True, 1)),
    "bound1.5-nomip": (1.5, False, (False, False, 1)),
}


@functools.lru_cache(maxsize=None)
def density_grid(kind, bound):
    """Built once per (scene, bound) and shared by the cases; never written to."""
    grid = (scene.brick_density_grid if kind == "bricks" else scene.sparse_density_grid)(bound=bound)
    grid.setflags(write=False)
    return grid


def march_variants(names):
    """The k_frame_march instantiations among a profiler's kernel names, demangled or not, as (MIP, POW2, MODE)."""
    out = set()
    for n in names:
        for mip, pow2, mode in re.findall(r"k_frame_march<(true|false), (true|false), (\d)>", n):
            out.add((mip == "true", pow2 == "true", int(mode)))
        for mip, pow2, mode in re.findall(r"k_frame_marchILb([01])ELb([01])ELi(\d)E", n):
            out.add((mip == "1", pow2 == "1", int(mode)))
    return out


def test_march_variants_reads_both_spellings():
    assert march_variants(["void pnr::k_frame_march<true, false, 1>(pnr::FrameCtl const*, pnr::FrameCtl*)", "pnr::k_frame_begin(int)"]) == {(True, False, 1)}
    assert march_variants(["_ZN3pnr13k_frame_marchILb0ELb1ELi1EEEvPKNS_8FrameCtlEPS1_", "_ZN3pnr13k_frame_marchILb1ELb1ELi2EEEvPKNS_8FrameCtlEPS1_"]) == {(False, True, 1), (True, True, 2)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("model_kind", ["nerf", "palette"])
def test_native_loop_matches_reference_style_loop_off_the_power_of_two_path(cuda, monkeypatch, model_kind, config):
    from torch.profiler import ProfilerActivity, profile
    bound, use_mip, variant = CONFIGS[config]
    monkeypatch.setattr(raymarching, "USE_MIP", use_mip)       # (restored by the fixture)
    lib = _lib.load()
    if model_kind == "nerf":
        m = network.NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1.0, min_near=0.2)
    else:
        m = network.PaletteNetwork(renderer.default_opt(), bound=bound, cuda_ray=True, density_scale=1.0, min_near=0.2)
    assert m.cascade == (3 if bound == 3.0 else 2)
    scene.seed_field_(m, 11)
    m = m.to(cuda).eval()
    m.count_rendered = True
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(48, 48), 48, 48)
    ro, rd = ro.to(cuda), rd.to(cuda)
    names = []

    def put(kind, density_scale):
        m.density_grid.copy_(torch.tensor(density_grid(kind, bound), device=cuda))
        raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
        m.density_scale = density_scale
        assert (raymarching.occupancy_mip(m.density_bitfield, m.cascade, m.grid_size, m.bound) is not None) == use_mip

    def native(ro_, rd_, **kw):
        m.march_mode, m.fused_field = "native", True
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            with torch.no_grad():
                r = m.render(ro_, rd_, perturb=False, T_thresh=1e-4, **kw)
            torch.cuda.synchronize()
        names.extend(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return r

    def both(ro_, rd_, **kw):
        m.march_mode, m.fused_field = "compat", False
        with torch.no_grad():
            a = m.render(ro_, rd_, perturb=False, T_thresh=1e-4, **kw)
        b = native(ro_, rd_, **kw)
        print(f"{model_kind} {config} N={ro_.shape[1]} {kw}: rendered {int(a['rendered'].item())} / {int(b['rendered'].item())}, iterations {b['iterations']}, "
              f"image err {float((b['image'] - a['image']).abs().max()):.3g}, weights_sum err {float((b['weights_sum'] - a['weights_sum']).abs().max()):.3g}, "
              f"depth err {float(torch.nan_to_num(b['depth'] - a['depth']).abs().max()):.3g}")
        assert int(a["rendered"].item()) == int(b["rendered"].item()), kw      # the sharp check on the march: the same samples
        assert torch.equal(torch.isnan(a["depth"]), torch.isnan(b["depth"])), kw
        for k in ("image", "weights_sum"):
            close(b[k], a[k].cpu().numpy(), tol=TOL, what=k)
        close(b["depth"], a["depth"].cpu().numpy(), tol=DEPTH_TOL, what="depth")
        return a, b

    # density_scale 1, constant steps: the whole frame, one ray, fewer rays than a wave
    put("bricks", 1.0)
    a, full = both(ro, rd, dt_gamma=0, max_steps=1024)
    assert int(full["rendered"].item()) > 1000
    both(ro[:, 1000:1001].contiguous(), rd[:, 1000:1001].contiguous(), dt_gamma=0, max_steps=1024)
    a, b = both(ro[:, 1000:1007].contiguous(), rd[:, 1000:1007].contiguous(), dt_gamma=0, max_steps=1024)
    assert int(b["rendered"].item()) > 100
    # ... and without the wave-cooperative march tail, which is compiled per variant too: the same bits
    try:
        assert lib.pnr_set_option(b"coop_march", 0) == 0
        c = native(ro, rd, dt_gamma=0, max_steps=1024)
    finally:
        lib.pnr_set_option(b"coop_march", 1)
    assert int(c["rendered"].item()) == int(full["rendered"].item())
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(torch.nan_to_num(c[k], nan=-7.0), torch.nan_to_num(full[k], nan=-7.0)), k
    # a step budget of 16 ends the loop
    a, b = both(ro, rd, dt_gamma=0, max_steps=16)
    assert int(b["rendered"].item()) > 0
    # translucent, growing steps, a scene that is mostly air: a handful of iterations (6 or 7), every ray alive to the end of its walk
    put("sparse", 0.02)
    a, b = both(ro, rd, dt_gamma=1.0 / 128, max_steps=1024)
    assert int(b["rendered"].item()) > 1000
    # dense enough for rays to end on T_thresh (at density_scale 1 this seeded field lets every ray walk to the far side, ~140 iterations): the
    # alive list shrinks and n_step grows to 8 while the loop runs on
    put("bricks", 30.0)
    a, b = both(ro, rd, dt_gamma=0, max_steps=1024)
    assert 1000 < int(b["rendered"].item()) < int(full["rendered"].item())

    ran = march_variants(names)
    assert ran == {variant}, (ran, sorted(set(n for n in names if "k_frame" in n)))
    assert (True, True, 2) not in ran
