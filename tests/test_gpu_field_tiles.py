"""The NeRF frame loop's field launch deals 32-row wave tiles to its waves one by one (csrc/frame_plan.hpp: field_wave_tile), counts the
survivors of the one-sample-per-ray iterations with one atomic add per wave tile and meets block-wide only once, for the weights.  Frames
through m.render on the native loop, composited inside the field kernel (composite_fusion 2) against the same loop with the separate
k_frame_composite launch compositing and counting (composite_fusion 0): bit for bit, and the same bits on every repetition."""
import warnings

import pytest
import torch

from palettenerf_amd import network, raymarching, scene

pytestmark = pytest.mark.gpu

KEYS = ("image", "depth", "weights_sum")


def _full_grid_(m, cuda):
    """Every cell of every cascade occupied: each ray that meets the box is alive in iteration 0 and emits a sample there."""
    m.density_grid.fill_(1.0)
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)


def _native(m, cuda):
    from palettenerf_amd.fused import NeRFFieldFused
    m = m.to(cuda).eval()
    _full_grid_(m, cuda)
    m.count_rendered = True
    m.march_mode, m.fused_field = "native", True
    m._fused = NeRFFieldFused(m)
    return m


@pytest.fixture(scope="module")
def model(cuda):
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 23)
    return _native(m, cuda)


@pytest.fixture(scope="module")
def rays(cuda):
    made = {}

    def get(H, W):
        if (H, W) not in made:
            pose = torch.from_numpy(scene.lookat_pose())[None]
            ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
            made[(H, W)] = (ro.to(cuda), rd.to(cuda))
        return made[(H, W)]
    return get


def _render(m, ro, rd, max_steps=1024):
    with torch.no_grad():
        return m.render(ro, rd, perturb=False, dt_gamma=0, max_steps=max_steps, T_thresh=1e-4)


def _same(a, b, what):
    assert int(a["rendered"].item()) == int(b["rendered"].item()), what
    assert a["iterations"] == b["iterations"], what
    for k in KEYS:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (what, k)


def _fused_against_composite_launch(lib, m, ro, rd, what):
    """composite_fusion 0 once (the reference of the case), composite_fusion 2 three times.  Returns the reference."""
    try:
        assert lib.pnr_set_option(b"composite_fusion", 0) == 0
        want = _render(m, ro, rd)
        assert lib.pnr_set_option(b"composite_fusion", 2) == 0
        for rep in range(3):
            _same(_render(m, ro, rd), want, (what, rep))
    finally:
        lib.pnr_set_option(b"composite_fusion", 2)
    return want


# 5 x 7: a full and a partial wave tile, six waves of workgroup 0 with nothing to do but the rendezvous for the weights.  100 x 90: the last chunk of the alive list partial.
# 364 x 364 = 132 496 rays: more than 512 * 8 wave tiles, the waves loop and their last round is partial.
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("density", [100.0, 0.05])
@pytest.mark.parametrize("H,W", [(5, 7), (100, 90), (364, 364)])
def test_field_wave_tiles_composite_as_the_composite_launch_does(cuda, model, rays, H, W, density, precision):
    """Opaque (density_scale 100: one sample per ray in nearly every iteration, the atomic survivor counts) and translucent (0.05: n_step climbs
    through 2, 3, 5 ... 8, wave tiles of 32, 30 and 28 rows that straddle chunk boundaries)."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = model
    m.density_scale = density
    m._fused.precision = precision
    ro, rd = rays(H, W)
    want = _fused_against_composite_launch(lib, m, ro, rd, (H, W, density, precision))
    assert int(want["rendered"].item()) >= H * W // 2 and float(want["weights_sum"].max()) > 0
    if density < 1:
        assert want["iterations"] > 30
    elif H * W > 131072:
        first = _render(m, ro, rd, max_steps=1)      # the frame's first iteration alone: its live rows
        assert first["iterations"] >= 1 and int(first["rendered"].item()) >= 131073


def test_field_wave_tiles_with_the_overflow_watch(cuda, rays):
    """The CHECK = true instantiation: the weight recipe of the frame queue's overflow case (tests/test_gpu_frames.py: _queue_model) at row_scale 300
    instead of 4e4 -- the static bound on the hidden activations fails, so the frame loop keeps split-fp16 and watches its operands, and no
    activation comes near fp16's range, so the frame stands as the watching kernel rendered it."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 11)
    row_scale = 300.0
    with torch.no_grad():
        m.sigma_net[1].weight[1:].mul_(64.0)
        m.color_net[0].weight[:, 16:].mul_(1.0 / 64.0)
        m.color_net[0].weight[5, 16:].mul_(64.0)
        m.color_net[0].weight[5].mul_(row_scale)
        m.color_net[1].weight[:, 5].mul_(1.0 / row_scale)
    m = _native(m, cuda)
    m._fused.precision = 1
    assert m._fused.frame_precision() == (1, True)
    ro, rd = rays(100, 90)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fp16's range.*")       # an overflow report would render the frame again in fp32
        want = _fused_against_composite_launch(lib, m, ro, rd, "watch")
    assert m._fused.frame_precision() == (1, True)
    assert int(want["rendered"].item()) >= 100 * 90 // 2 and float(want["weights_sum"].max()) > 0
