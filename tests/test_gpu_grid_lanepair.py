"""The lane-pair form of the frame loop's level-major lookup (frame.hip: grid_pair_level, pnr_set_option("grid_lane_pairs")) against the same frame with it
switched off: lanes 2k and 2k + 1 still own rows b and b + 1 but split the loads by the corners' x bit and hand each other four values per level over DPP.
The encoder output must be grid_row's bit for bit, so every output of the frame, its sample count and its iteration count must be equal to the bit."""
import pytest
import torch

from palettenerf_amd import network, raymarching, scene

pytestmark = pytest.mark.gpu

LAYOUTS = ["single"]   # the table layouts that have the form (frame.hip: k_frame_grid_lp)
KEYS = ("image", "depth", "weights_sum", "rendered", "iterations")
DEFAULT = 1   # the shipped default of grid_lane_pairs (raymarch.hip), restored after every case


def _model(cuda, layout, density_scale, scene_kind):
    from palettenerf_amd.fused import NeRFFieldFused
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2)
    scene.seed_field_(m, 3)
    m = m.to(cuda).eval()
    grid = scene.brick_density_grid() if scene_kind == "bricks" else scene.sparse_density_grid()
    m.density_grid.copy_(torch.from_numpy(grid).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field, m.count_rendered = "native", True, True
    m._fused = NeRFFieldFused(m)
    m._fused.table_half = layout.startswith("half")
    return m


def _rays(cuda, H, W, azimuth_deg=70.0):
    pose = torch.from_numpy(scene.lookat_pose(azimuth_deg=azimuth_deg))[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro.to(cuda), rd.to(cuda)


def _keep(r):
    return {k: torch.as_tensor(r[k]).clone() for k in KEYS}


def _same(a, b, what=""):
    assert int(a["rendered"]) == int(b["rendered"]) > 1000, what
    assert int(a["iterations"]) == int(b["iterations"]), what
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (what, k)


def _both(lib, m, ro, rd, **kw):
    out = []
    try:
        for pairs in (0, 1):
            assert lib.pnr_set_option(b"grid_lane_pairs", pairs) == 0
            with torch.no_grad():
                out.append(_keep(m.render(ro, rd, perturb=False, max_steps=1024, T_thresh=1e-4, **kw)))
    finally:
        lib.pnr_set_option(b"grid_lane_pairs", DEFAULT)
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("density_scale", [1.0, 0.05])
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
@pytest.mark.parametrize("scene_kind", ["bricks", "sparse"])
def test_lane_pair_lookup_is_bit_identical(cuda, layout, scene_kind, dt_gamma, density_scale):
    """Dense and sparse scenes, constant and growing steps; the opaque field runs n_step = 1 (a pair is two neighbouring rays), the translucent one reaches
    n_step 3, 5 and 7: there a pair spans two rays and dead slots (delta == 0) sit next to live ones."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = _model(cuda, layout, density_scale, scene_kind)
    ro, rd = _rays(cuda, 160, 200)
    a, b = _both(lib, m, ro, rd, dt_gamma=dt_gamma)
    _same(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("density_scale,scene_kind", [(1.0, "bricks"), (0.05, "sparse")])
def test_lane_pair_lookup_next_to_hosted_rows(cuda, layout, density_scale, scene_kind):
    """hosted_tail on with a march budget of one probe: most rows of a launch are flagged for the hosted workgroups (rowflag), so most pairs have one
    flagged partner -- it gets no loads and no store from the pair, and the hosted tail's own lookups write it."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = _model(cuda, layout, density_scale, scene_kind)
    ro, rd = _rays(cuda, 160, 200)
    try:
        assert lib.pnr_set_option(b"hosted_tail", 1) == 0 and lib.pnr_set_option(b"march_budget", 1) == 0 and lib.pnr_set_option(b"march_budget0", 1) == 0
        a, b = _both(lib, m, ro, rd, dt_gamma=0.0)
    finally:
        lib.pnr_set_option(b"hosted_tail", 1); lib.pnr_set_option(b"march_budget", 2); lib.pnr_set_option(b"march_budget0", 0)
    _same(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_lane_pair_lookup_odd_row_count(cuda, layout):
    """159 x 201 rays: an odd count; with n_step = 1 the last row of a launch has no partner (b + 1 is out of range and is neither read nor written)."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = _model(cuda, layout, 1.0, "bricks")
    ro, rd = _rays(cuda, 159, 201)
    assert ro.shape[1] % 2 == 1
    a, b = _both(lib, m, ro, rd, dt_gamma=0.0)
    _same(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("submit_value", [0, 1])
def test_lane_pair_option_is_read_at_submit(cuda, layout, submit_value):
    """render_prepare / render_launch / render_finish with grid_lane_pairs flipped between launch and finish: the frame's plan holds the kernel it was
    submitted with (make_frame_plan), the chunks the finish call enqueues run it too, and the frame equals the frame rendered whole at the submit-time value."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    m = _model(cuda, layout, 1.0, "bricks")
    ro, rd = _rays(cuda, 160, 200)
    pose = torch.from_numpy(scene.lookat_pose_from((3.0, 1.0, 0.5), target=(6.0, 2.5, 0.5)))[None]   # looks past the object: a few iterations
    so, sd = scene.get_rays(pose, scene.intrinsics_from_fov(160, 200), 160, 200)
    so, sd = so.to(cuda), sd.to(cuda)
    kw = dict(perturb=False, dt_gamma=0.0, max_steps=1024, T_thresh=1e-4)
    try:
        assert lib.pnr_set_option(b"grid_lane_pairs", submit_value) == 0
        with torch.no_grad():
            want = _keep(m.render(ro, rd, **kw))
            m.render(so, sd, **kw)   # this thread's iteration prediction: short -> the submit call of the next frame enqueues only its first iterations
            pend = m.render_launch(m.render_prepare(ro, rd, **kw))
            assert lib.pnr_set_option(b"grid_lane_pairs", 1 - submit_value) == 0
            got = _keep(m.render_finish(pend))
    finally:
        lib.pnr_set_option(b"grid_lane_pairs", DEFAULT)
    _same(want, got, submit_value)
