"""Host side of the guard-band tests: tests/guarded.py tests itself on CPU tensors, and the inventory -- every pnr_* function of include/pnr.h is
classified, every entry classified `guarded` is called by a case of tests/test_gpu_guard_bands.py, and nothing on the training step or the frame
loop is classified otherwise."""
import os
import re

import pytest
import torch

from tests import guarded
from tests import test_gpu_guard_bands as cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---------------------------------------------------------------- the helper on CPU tensors
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int32, torch.uint8])
@pytest.mark.parametrize("align", [0, 256, 4, 16, 252])
def test_out_places_the_view_and_reports_strays_with_their_offsets(dtype, align):
    size = torch.empty((), dtype=dtype).element_size()
    buf, view = guarded.out((7, 3), dtype, "cpu", align)
    nbytes = 21 * size
    assert view.shape == (7, 3) and view.dtype == dtype and view.is_contiguous()
    assert view.data_ptr() % 256 == align % 256
    start = view.data_ptr() - buf.data_ptr()
    assert start >= guarded.GUARD and buf.numel() - start - nbytes >= guarded.GUARD      # at least 64 KiB in front and behind
    assert bool((buf == guarded.SENTINEL).all())
    view.zero_()
    view.view(-1)[-1] = 1                           # the "kernel" writes the view's last element: not a stray
    assert guarded.untouched(buf, view) and guarded.first_touched(buf) is None
    flat = buf[start - size:start + nbytes + size].view(dtype)      # the view with one element in front and one behind
    flat[-1] = 0                                    # one element behind the end
    assert not guarded.untouched(buf, view)
    assert guarded.first_touched(buf) == nbytes and "0 bytes behind the end" in guarded.last_report
    flat[-1] = flat[-2] = 0
    buf[start + nbytes:start + nbytes + size] = guarded.SENTINEL
    assert guarded.untouched(buf, view)
    flat[0] = 0                                     # one element in front
    assert not guarded.untouched(buf, view)
    assert guarded.first_touched(buf) == -size and f"{size} bytes in front" in guarded.last_report
    buf[start - size:start] = guarded.SENTINEL
    buf[start + nbytes + 12] = 0                    # "12 bytes behind the end"
    assert not guarded.untouched(buf, view) and guarded.first_touched(buf) == nbytes + 12 and "12 bytes behind the end" in guarded.last_report


def test_back_guard_starts_at_the_byte_after_the_last_element_of_an_odd_sized_view():
    buf, view = guarded.out((3, 5), torch.uint8, "cpu", 1)      # 15 bytes, starting at an odd address
    assert view.data_ptr() % 256 == 1
    start = view.data_ptr() - buf.data_ptr()
    view.fill_(7)
    assert int(buf[start + 14]) == 7 and int(buf[start + 15]) == guarded.SENTINEL and int(buf[start - 1]) == guarded.SENTINEL
    buf[start + 15] = 7                             # the very next byte
    assert not guarded.untouched(buf, view) and guarded.first_touched(buf) == 15
    ws_buf, ws = guarded.workspace(1001, "cpu", 16)             # exactly the bytes asked for, not rounded up
    assert ws.numel() == 1001 and ws.dtype == torch.uint8 and ws.data_ptr() % 256 == 16
    ws.zero_()
    assert guarded.untouched(ws_buf, ws)
    ws_buf[ws.data_ptr() - ws_buf.data_ptr() + 1001] = 0
    assert not guarded.untouched(ws_buf, ws) and guarded.first_touched(ws_buf) == 1001


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("align", [0, 4, 16])
def test_inp_surrounds_a_floating_array_with_nans(dtype, align):
    t = torch.arange(10, dtype=dtype).view(5, 2)
    buf, view = guarded.inp(t, align)
    size = t.element_size()
    assert torch.equal(view, t) and view.data_ptr() % 256 == align % 256
    start = view.data_ptr() - buf.data_ptr()
    around = buf[start - 64 * size:start + 10 * size + 64 * size].view(dtype)
    assert bool(torch.isnan(around[:64]).all()) and bool(torch.isnan(around[74:]).all()) and torch.equal(around[64:74], t.view(-1))
    assert bool(torch.isnan(buf[:start - start % size].view(dtype)).all())
    assert guarded.untouched(buf, view)
    around[74] = 0
    assert not guarded.untouched(buf, view) and guarded.first_touched(buf) == 10 * size


def test_inp_surrounds_an_index_array_with_values_of_its_meaning():
    rays = torch.tensor([[3, 0, 7], [1, 7, 2]], dtype=torch.int32)
    buf, view = guarded.inp(rays, 4, around=(0, 0, 1))
    assert torch.equal(view, rays) and view.data_ptr() % 256 == 4
    start = view.data_ptr() - buf.data_ptr()
    rows = buf[start - 120:start + 24 + 120].view(torch.int32).view(-1, 3)
    assert rows[:10].tolist() == [[0, 0, 1]] * 10 and rows[12:].tolist() == [[0, 0, 1]] * 10     # whole triples end at the view and begin behind it
    assert guarded.untouched(buf, view)
    rows[12, 2] = 5
    assert not guarded.untouched(buf, view) and guarded.first_touched(buf) == 24 + 8
    with pytest.raises(ValueError):
        guarded.inp(rays)                           # never a bit pattern around an index array
    bits, v = guarded.inp(torch.arange(9, dtype=torch.uint8), 1, around=0x00)      # integers that are data, not indices: a byte
    assert v.data_ptr() % 256 == 1 and int(bits[v.data_ptr() - bits.data_ptr() + 9]) == 0 and guarded.untouched(bits, v)


# ---------------------------------------------------------------- the inventory
G = "guarded"
NO_PTR = "no device pointer"
LEFT = "left out: "
# the families the training step and the frame loop call: none of these may be classified anything but guarded
REQUIRED = (
        "pnr_mlp_forward", "pnr_mlp_backward", "pnr_mlp_forward_lm", "pnr_mlp_backward_lm", "pnr_mlp_pack",
        "pnr_grid_encode_forward", "pnr_grid_encode_forward_layout", "pnr_grid_encode_forward_pair", "pnr_grid_encode_backward", "pnr_grid_encode_backward_binned",
        "pnr_sh_encode_forward", "pnr_sh_encode_backward", "pnr_sh_encode_cat_forward", "pnr_sigma_geo_cat_forward", "pnr_sigma_geo_cat_backward",
        "pnr_composite_rays_train_forward", "pnr_composite_rays_train_backward", "pnr_composite_rays_train_norm_forward",
        "pnr_composite_rays_train_norm_backward", "pnr_composite_rays_flex_train_forward", "pnr_composite_rays_flex_train_backward", "pnr_spread_ray_to_sample",
        "pnr_composite_rays", "pnr_composite_rays_flex", "pnr_composite_rays_flex_multi", "pnr_march_rays", "pnr_march_rays_mip", "pnr_march_rays_fill",
        "pnr_march_rays_train", "pnr_march_rays_train_mip", "pnr_build_occupancy_mip", "pnr_compact_alive", "pnr_near_far_from_aabb", "pnr_packbits",
        "pnr_morton3d", "pnr_morton3d_invert",
        "pnr_adam_step", "pnr_adam_step_amp", "pnr_grad_check", "pnr_ema_update", "pnr_ema_swap",
        "pnr_linear_wgrad", "pnr_linear_bgrad",
        "pnr_palette_heads_forward", "pnr_palette_heads_backward", "pnr_palette_train_shade_forward", "pnr_palette_train_shade_backward",
        "pnr_palette_smooth_points", "pnr_palette_smooth_forward", "pnr_palette_smooth_backward", "pnr_train_loss_forward", "pnr_train_loss_backward",
        "pnr_train_loss_backward_bg",
        "pnr_nerf_field_forward", "pnr_nerf_density_forward", "pnr_palette_field_forward", "pnr_background_forward", "pnr_background_train_forward",
        "pnr_background_backward",
        "pnr_nerf_render_frame", "pnr_palette_render_frame")
INVENTORY = {
    # host only
    "pnr_error_string": NO_PTR, "pnr_abi_version": NO_PTR, "pnr_set_option": NO_PTR, "pnr_scan_scratch_bytes": NO_PTR, "pnr_occupancy_mip_bytes": NO_PTR,
    "pnr_occupancy_workspace_bytes": NO_PTR, "pnr_occupancy_samples": NO_PTR, "pnr_nerf_field_packed_bytes": NO_PTR, "pnr_nerf_frame_workspace_bytes": NO_PTR,
    "pnr_palette_frame_workspace_bytes": NO_PTR, "pnr_palette_field_stages_aux": NO_PTR, "pnr_palette_field_packed_bytes": NO_PTR,
    "pnr_palette_aux_channels": NO_PTR, "pnr_grid_backward_binned_workspace_bytes": NO_PTR, "pnr_linear_wgrad_workspace_bytes": NO_PTR,
    "pnr_mlp_packed_bytes": NO_PTR, "pnr_mlp_backward_workspace_bytes": NO_PTR, "pnr_adam_max_tensors": NO_PTR,
    "pnr_palette_train_shade_workspace_bytes": NO_PTR, "pnr_train_loss_workspace_bytes": NO_PTR, "pnr_background_packed_bytes": NO_PTR,
    "pnr_background_backward_workspace_bytes": NO_PTR, "pnr_launch_geometry": NO_PTR, "pnr_lattice_density_workspace_bytes": NO_PTR,
    "pnr_mesh_case_triangles": NO_PTR, "pnr_mesh_workspace_bytes": NO_PTR, "pnr_frame_metrics_workspace_bytes": NO_PTR, "pnr_mesh_vertex_record_bytes": NO_PTR,
    "pnr_extract_kmeans_workspace_bytes": NO_PTR,
    # the training step and the frame loop
    **{name: G for name in REQUIRED},
    # what the guarded cases need on the way: the packers (their blobs are guarded at exactly *_packed_bytes), the interleaved tables, the sphere coordinates
    "pnr_nerf_field_pack": G, "pnr_palette_field_pack": G, "pnr_background_pack": G,
    "pnr_interleave_tables": G, "pnr_interleave_tables3": G, "pnr_interleave_tables3_half": G, "pnr_sph_from_ray": G,
    # guarded by the tests of their own tools
    "pnr_palette_sheets": "elsewhere:tests/test_gpu_evaluate.py", "pnr_lut_weights": "elsewhere:tests/test_gpu_lut.py",
    # offline tools and one-off launches outside the training step and the frame loop
    "pnr_nerf_render_frame_submit": LEFT + "the two-call form of pnr_nerf_render_frame: the same launches on the same workspace, the one-call form is guarded",
    "pnr_nerf_render_frame_finish": LEFT + "see pnr_nerf_render_frame_submit",
    "pnr_palette_render_frame_submit": LEFT + "the two-call form of pnr_palette_render_frame, whose one-call form is guarded",
    "pnr_palette_render_frame_finish": LEFT + "see pnr_palette_render_frame_submit",
    "pnr_occupancy_update": LEFT + "occupancy update: every 16th step, off the step's critical path", "pnr_occupancy_begin": LEFT + "occupancy update",
    "pnr_occupancy_points": LEFT + "occupancy update", "pnr_occupancy_scatter": LEFT + "occupancy update", "pnr_occupancy_commit": LEFT + "occupancy update",
    "pnr_mark_untrained_grid": LEFT + "occupancy update: once per run",
    "pnr_checksum": LEFT + "checksum: cache guard, reads whole buffers the caller sizes", "pnr_get_rays": LEFT + "get_rays: ray generation, once per frame or batch",
    "pnr_image_to_uint8": LEFT + "image_to_uint8: the writer's last step", "pnr_present_frame": LEFT + "present: the viewer's step behind a frame",
    "pnr_rgb_to_hsv": LEFT + "hsv: palette tool", "pnr_hsv_to_rgb": LEFT + "hsv: palette tool", "pnr_rgb_histogram": LEFT + "histogram: palette extraction",
    "pnr_lattice_points": LEFT + "lattice: mesh export", "pnr_lattice_density": LEFT + "lattice: mesh export", "pnr_mesh_count": LEFT + "mesh export",
    "pnr_mesh_emit": LEFT + "mesh export", "pnr_density_gradient": LEFT + "normals: mesh export", "pnr_mesh_vertex_records": LEFT + "mesh export",
    "pnr_frame_metrics": LEFT + "metrics: evaluation loop", "pnr_train_batch": LEFT + "train batch: data loading, its own float64 tests",
    "pnr_error_map_update": LEFT + "error map: data loading", "pnr_stylizer_fit": LEFT + "stylizer: the GUI's optimise step",
    "pnr_extract_accumulate": LEFT + "extract: palette extraction", "pnr_extract_kmeans": LEFT + "extract: palette extraction",
}


def header_functions():
    text = open(os.path.join(ROOT, "include", "pnr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(pnr_\w+)\s*\(", text))


def test_every_entry_of_the_header_is_classified():
    declared = header_functions()
    assert len(declared) > 100
    assert declared - set(INVENTORY) == set(), "new entry points: classify them in INVENTORY (and guard what a training step or a frame calls)"
    assert set(INVENTORY) - declared == set(), "INVENTORY names functions the header does not declare"
    for name, kind in INVENTORY.items():
        assert kind in (G, NO_PTR) or kind.startswith(LEFT) or kind.startswith("elsewhere:"), name
        if kind.startswith("elsewhere:"):
            path = os.path.join(ROOT, kind.split(":", 1)[1])
            assert os.path.exists(path) and name in open(path).read(), f"{name}: {kind} does not call it"


def test_every_guarded_entry_is_called_by_a_case_and_the_required_families_are_guarded():
    guarded_names = {name for name, kind in INVENTORY.items() if kind == G}
    assert guarded_names - set(cases.ENTRIES) == set(), "classified guarded, but no case of tests/test_gpu_guard_bands.py registers them"
    assert set(cases.ENTRIES) - guarded_names == set(), "registered by a case, but not classified guarded"
    for name, tests in cases.ENTRIES.items():
        assert tests and all(hasattr(cases, t) for t in tests), name
    assert len(REQUIRED) == 61 and all(INVENTORY[name] == G for name in REQUIRED)
