"""dropin.fuse_loop on the device: an unchanged reference-style caller -- a plain nn.Module that carries what the reference's constructors define and
whose class-level run_cuda must never be reached -- renders its inference frames through the native frame call.

Two yardsticks per frame:
  * the mirror model's own native run_cuda on the same rays (the same entry point with the same arguments: equality is exact, bit for bit);
  * the reference-driven golden frames, at the tolerances tests/test_gpu_frames.py, test_gpu_fp16_clip.py, test_gpu_jitter.py and
    test_gpu_background.py apply to the mirror's native loop against the same files (imported from there)."""
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from palettenerf_amd import dropin, network, raymarching, renderer, scene
from tests import test_gpu_background as tbg
from tests import test_gpu_fp16_clip as tclip
from tests import test_gpu_jitter as tjit
from tests.test_gpu_frames import COLOUR_TOL, DEPTH_TOL, EDIT_TOL, close, frame_rays, load, put_scene
from tests.test_host_logic import _extra_model, set_extra_edit, set_extra_stylizer

pytestmark = pytest.mark.gpu

NERF_KEYS = ["depth", "image", "rgb_norm", "weights_sum"]                                           # nerf/renderer.py:388-391
GUI_KEYS = ["depth", "depth_origin", "image", "weights_sum", "clip_feat"]                             # palette/renderer.py:531-537
FULL_KEYS = GUI_KEYS + ["direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"]  # palette/renderer.py:546-550
KW = dict(perturb=False, max_steps=1024, T_thresh=1e-4)

# what NeRFRenderer / PaletteRenderer.__init__ and the two network constructors of the reference set on `self` besides modules and buffers
RENDERER_SCALARS = ["bound", "cascade", "grid_size", "density_scale", "min_near", "density_thresh", "bg_radius", "cuda_ray", "mean_density", "iter_density",
                    "mean_count", "local_step"]
NETWORK_SCALARS = ["num_layers", "hidden_dim", "geo_feat_dim", "in_dim", "num_layers_color", "hidden_dim_color", "in_dim_dir"]
BG_SCALARS = ["num_layers_bg", "hidden_dim_bg", "in_dim_bg"]
PALETTE_SCALARS = ["num_basis", "freeze_basis_color", "require_smooth_loss", "color_weight", "edit", "stylizer", "view_dep_weight", "offsets_weight",
                   "in_dim_palette", "in_dim_clip"]
BUFFERS = ["aabb_train", "aabb_infer", "density_grid", "density_bitfield", "step_counter"]           # tests/golden/state_dict_layout.json


class Reached(Exception):
    pass


class Caller(nn.Module):
    """The reference-style caller: NOT derived from this package's renderer classes, with the attributes the reference's constructors define (copied
    from a mirror model: modules and parameters deep-copied, buffers cloned) and none of the mirror's own (march_mode, fused_field, _fused, ...)."""

    def __init__(self, src):
        super().__init__()
        palette = hasattr(src, "encoder_palette")
        names = RENDERER_SCALARS + NETWORK_SCALARS + (BG_SCALARS if src.bg_radius > 0 else []) + (PALETTE_SCALARS if palette else [])
        for name in names:
            setattr(self, name, getattr(src, name))
        for name in BUFFERS:
            self.register_buffer(name, getattr(src, name).clone())
        for name, module in src.named_children():
            setattr(self, name, copy.deepcopy(module))
        if src.bg_net is None:
            self.bg_net = None
        if palette:
            self.opt = copy.copy(src.opt)
            self.basis_color = nn.Parameter(src.basis_color.detach().clone())
        self.train(src.training)
        self.reached = 0

    def run_cuda(self, rays_o, rays_d, **kwargs):
        self.reached += 1
        raise Reached("the class's own run_cuda")

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):     # nerf/renderer.py:564-603 for a cuda_ray model
        return self.run_cuda(rays_o, rays_d, **kwargs)

    def background(self, x, d):                                                       # nerf/network.py:145-160
        self.background_calls = getattr(self, "background_calls", 0) + 1
        h = torch.cat([self.encoder_dir(d), self.encoder_bg(x)], dim=-1)
        for l in range(self.num_layers_bg):
            h = self.bg_net[l](h)
            if l != self.num_layers_bg - 1:
                h = F.relu(h, inplace=True)
        return torch.sigmoid(h)


def caller_of(src):
    c = Caller(src)
    assert not isinstance(c, renderer._RendererBase)
    for name in ("march_mode", "fused_field", "_fused", "_bg_fused", "_native_frame", "_background_of_rays", "count_rendered"):
        assert not hasattr(c, name), name
    assert dropin.fuse_loop(c) is c and type(c).run_cuda is Caller.run_cuda
    return c


def go_native(m):
    m.march_mode, m.fused_field = "native", True
    return m


def mirror(kind, cuda, seed=0, density_scale=1.0, pred_clip=False, grid=None, **kw):
    if kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2, **kw)
    else:
        m = network.PaletteNetwork(renderer.default_opt(pred_clip=pred_clip), bound=2, cuda_ray=True, density_scale=density_scale, min_near=0.2, **kw)
    scene.seed_field_(m, seed)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid() if grid is None else grid).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return go_native(m)


def golden_mirror(kind, cuda, g):
    return mirror(kind, cuda, int(g["seed"]), float(g["density_scale"]), bool(g["pred_clip"]) if kind == "palette" else False)


def rays(cuda, H, W, azimuth=45.0):
    pose = torch.from_numpy(scene.lookat_pose(azimuth_deg=azimuth))[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro.to(cuda), rd.to(cuda)


def identical(got, want, keys, what=""):
    """Bit for bit (NaN == NaN: the depth of a ray that misses the box is 0 / 0 in the reference too), same shape, fp32; and the same march."""
    for k in keys:
        a, b = got[k], want[k]
        assert a.dtype == torch.float32 and a.shape == b.shape, (what, k, a.dtype, a.shape, b.shape)
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), (what, k)
    assert int(got["rendered"].sum()) == int(want["rendered"].sum()) and got["n_samples"] == want["n_samples"] and "iterations" in got, what


def keys_of(kind, gui_mode=False):
    return NERF_KEYS if kind == "nerf" else (GUI_KEYS if gui_mode else FULL_KEYS)


def gui(kind, on):
    return {"gui_mode": on} if kind == "palette" else {}


def frame(m, ro, rd, **kw):
    with torch.no_grad():
        return m.run_cuda(ro, rd, **kw)


# ---------------------------------------------------------------- 1. against the goldens and the mirror's native frame
@pytest.mark.parametrize("case", ["a", "b"])
def test_nerf_caller_frames(cuda, golden_dir, case):
    g = load(golden_dir, f"frame_nerf_{case}")
    m = golden_mirror("nerf", cuda, g)
    c = caller_of(m)
    ro, rd = frame_rays(g, cuda)
    kw = dict(dt_gamma=float(g["dt_gamma"]), workspace="unused", fp16=False, **KW)      # (callers pass **vars(opt): unknown keywords)
    with torch.no_grad():
        r = c.render(ro, rd, staged=True, **kw)
    close(r["image"], g["image"], what="image")
    close(r["weights_sum"], g["weights_sum"], what="weights_sum")
    close(r["depth"], g["depth"], tol=DEPTH_TOL, what="depth")
    identical(r, frame(m, ro, rd, **kw), NERF_KEYS)
    assert c.reached == 0 and not r["rgb_norm"].any()


@pytest.mark.parametrize("case", ["a", "b"])
def test_palette_caller_frames_all_maps_and_edit(cuda, golden_dir, case):
    g = load(golden_dir, f"frame_palette_{case}")
    m = golden_mirror("palette", cuda, g)
    c = caller_of(m)
    ro, rd = frame_rays(g, cuda)
    kw = dict(dt_gamma=float(g["dt_gamma"]), **KW)
    r = frame(c, ro, rd, gui_mode=False, **kw)
    for k in ("image", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
        close(r[k], g[k], what=k)
    close(r["depth"], g["depth"], tol=DEPTH_TOL, what="depth")
    close(r["depth_origin"], g["depth_origin"], tol=DEPTH_TOL, what="depth_origin")
    identical(r, frame(m, ro, rd, gui_mode=False, **kw), FULL_KEYS)
    for x in (m, c):
        x.edit = renderer.RegionEdit(x.opt)
        x.edit.update_cent(mean_xyz=torch.tensor([0.1, 0.0, -0.2], device=cuda))
        x.edit.update_std(std_xyz=0.5)
        x.edit.update_delta_hsv(x.basis_color.data.clamp(0, 1), (x.basis_color.data * 0.6 + 0.2).flip(0).clamp(0, 1))
    e = frame(c, ro, rd, gui_mode=True, **kw)
    close(e["image"], g["edit_image"], tol=EDIT_TOL, what="edit_image")
    assert "basis_rgb" not in e
    identical(e, frame(m, ro, rd, gui_mode=True, **kw), GUI_KEYS, "edit")
    assert c.reached == 0


@pytest.mark.parametrize("case", ["style_a", "style_b", "nb6", "nb8"])
def test_palette_caller_stylizer_edit_and_many_basis_frames(cuda, golden_dir, case):
    g = load(golden_dir, f"frame_palette_{case}")
    opt, m = _extra_model(g)
    m = go_native(m.to(cuda).eval())
    put_scene(m, cuda)
    c = caller_of(m)
    ro, rd = frame_rays(g, cuda)
    kw = dict(dt_gamma=float(g["dt_gamma"]), **KW)
    r = frame(c, ro, rd, gui_mode=False, **kw)
    for k in ("image", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
        close(r[k], g[k], what=k)
    close(r["depth"], g["depth"], tol=DEPTH_TOL, what="depth")
    identical(r, frame(m, ro, rd, gui_mode=False, **kw), FULL_KEYS)
    for x in (m, c):
        set_extra_stylizer(x, x.opt, g, cuda)
    s = frame(c, ro, rd, gui_mode=True, **kw)
    close(s["image"], g["style_image"], what="style_image")
    identical(s, frame(m, ro, rd, gui_mode=True, **kw), GUI_KEYS, "stylizer")
    assert c.reached == 0
    with pytest.raises(Reached):          # outside gui_mode the reference defines no basis maps for the Stylizer: the class's own method decides
        frame(c, ro, rd, gui_mode=False, **kw)
    assert c.reached == 1
    for x in (m, c):
        x.stylizer = None
        set_extra_edit(x, x.opt, cuda)
    e = frame(c, ro, rd, gui_mode=False, **kw)
    close(e["image"], g["edit_image"], tol=EDIT_TOL, what="edit_image")
    close(e["basis_rgb"], g["edit_basis_rgb"], tol=EDIT_TOL, what="edit_basis_rgb")
    identical(e, frame(m, ro, rd, gui_mode=False, **kw), FULL_KEYS, "edit")
    c.edit.weight_mode = True
    close(frame(c, ro, rd, gui_mode=True, **kw)["image"], g["edit_weight_image"], what="edit_weight_image")
    assert c.reached == 1


@pytest.mark.parametrize("case", ["a", "b"])
def test_palette_caller_under_fp16_autocast_with_the_clip_head(cuda, golden_dir, case):
    g = tclip.load(golden_dir, case)
    m = tclip.clip_model(cuda, int(g["seed"]), float(g["density_scale"]), float(g["scale"]))
    c = caller_of(m)
    ro, rd = tclip.rays(cuda, int(g["H"]), int(g["W"]))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        r = c.run_cuda(ro, rd, dt_gamma=float(g["dt_gamma"]), **tclip.KW)
    assert c._fused.table_half is False and c.reached == 0
    for k in tclip.MAPS:
        close(r[k], g[f"half_{k}"], tol=tclip.TOL, what=k)
    assert float(np.abs(r["image"].cpu().numpy() - g["fp32_image"]).max()) > 4 * tclip.TOL      # the half tables, not the fp32 ones
    identical(r, tclip.half_frame(m, ro, rd, dt_gamma=float(g["dt_gamma"])), FULL_KEYS)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_caller_jittered_frames(cuda, golden_dir, kind):
    g = tjit.load(golden_dir, kind, "a")
    m = tjit.golden_model(kind, cuda, g)
    c = caller_of(m)
    ro, rd = tjit.frame_rays(cuda, int(g["H"]), int(g["W"]))
    kw = dict(dt_gamma=float(g["dt_gamma"]), **gui(kind, True), **tjit.KW)
    for s in (2, 3):                       # the golden's own noise, passed through
        noises = torch.from_numpy(g[f"noises_s{s}"]).to(cuda)
        r = frame(c, ro, rd, perturb=s, noises=noises, **kw)
        for k in (tjit.NERF_KEYS if kind == "nerf" else tjit.GUI_KEYS):
            tjit.close(r[k], g[f"s{s}_{k}"], tjit.tol_of(k), f"{kind} seed {s} {k}")
        identical(r, frame(m, ro, rd, perturb=s, noises=noises, **kw), keys_of(kind, True), f"seed {s}")
    out = []
    for x in (c, m):                       # perturb alone: the one torch.rand(N) the per-op loop's first march draws
        torch.manual_seed(11)
        out.append(frame(x, ro, rd, perturb=True, **kw))
    identical(out[0], out[1], keys_of(kind, True), "perturb")
    torch.manual_seed(11)
    want = torch.rand(ro.shape[1], dtype=torch.float32, device=cuda)
    identical(out[0], frame(m, ro, rd, perturb=False, noises=want, **kw), keys_of(kind, True), "the draw")
    assert not torch.equal(out[0]["image"], frame(c, ro, rd, perturb=False, **kw)["image"]) and c.reached == 0


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_caller_frames_with_a_background_model(cuda, golden_dir, kind):
    g = tbg.golden(golden_dir, f"frame_bg_{kind}_a")
    m = tbg.golden_model(kind, cuda, g)
    c = caller_of(m)
    ro, rd = tbg.frame_rays(cuda, int(g["H"]), int(g["W"]))
    kw = dict(dt_gamma=float(g["dt_gamma"]), perturb=False, **gui(kind, False), **tbg.KW)
    r = frame(c, ro, rd, **kw)
    for k in (tbg.NERF_KEYS if kind == "nerf" else tbg.FULL_KEYS):
        tbg.close(r[k], g[k], tbg.tol_of(k), f"{kind} {k}")
    identical(r, frame(m, ro, rd, **kw), keys_of(kind))
    assert c.reached == 0 and not hasattr(c, "background_calls") and c.__dict__.get("_bg_fused") is not None     # the one-launch background
    dropin.unfuse(c)
    assert "_bg_fused" not in c.__dict__ and "_fused" not in c.__dict__ and "_loop" not in c.__dict__ and "run_cuda" not in c.__dict__


def test_a_background_of_another_architecture_goes_in_as_the_frames_bg_map(cuda):
    m = mirror("nerf", cuda, seed=5, density_scale=20.0, bg_radius=4, hidden_dim_bg=32)
    c = caller_of(m)
    ro, rd = rays(cuda, 24, 20)
    r = frame(c, ro, rd, **KW)
    assert c.background_calls == 1 and c.__dict__.get("_bg_fused") is None and c.reached == 0
    identical(r, frame(m, ro, rd, **KW), NERF_KEYS)
    c.bg_radius = 0
    white = frame(c, ro, rd, **KW)
    assert float((white["image"] - r["image"]).abs().max()) > 1e-2          # the background did reach the image


# ---------------------------------------------------------------- 2. keys, shapes, ragged sizes
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_reference_keys_and_prefix_shapes(cuda, kind):
    m = mirror(kind, cuda, seed=3, density_scale=20.0, pred_clip=True)
    c = caller_of(m)
    ro, rd = rays(cuda, 12, 10)
    N = ro.shape[1]
    nb, cd = (c.num_basis, c.opt.clip_dim) if kind == "palette" else (0, 0)
    shapes = {"depth": (), "depth_origin": (), "image": (3,), "rgb_norm": (), "clip_feat": (cd,), "direct_rgb": (3,), "view_dep_rgb": (3,),
              "basis_rgb": (3 * nb,), "unscaled_basis_rgb": (3 * nb,), "basis_acc": (nb,)}
    for prefix, o, d in (((1, N), ro, rd), ((N,), ro[0], rd[0]), ((2, N // 2), ro.view(2, N // 2, 3), rd.view(2, N // 2, 3))):
        for gui_mode in ((False, True) if kind == "palette" else (False,)):
            r = frame(c, o, d, **gui(kind, gui_mode), **KW)
            for k in keys_of(kind, gui_mode):
                want = (N,) if k == "weights_sum" else prefix + shapes[k]
                assert tuple(r[k].shape) == want and r[k].dtype == torch.float32 and r[k].device == o.device, (prefix, gui_mode, k, tuple(r[k].shape))
            if kind == "palette":
                assert ("basis_rgb" in r) == (not gui_mode)
            identical(r, frame(m, o, d, **gui(kind, gui_mode), **KW), keys_of(kind, gui_mode), (prefix, gui_mode))
    assert c.reached == 0


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_ragged_ray_counts(cuda, golden_dir, kind, n):
    g = load(golden_dir, f"frame_{kind}_a")
    m = golden_mirror(kind, cuda, g)
    c = caller_of(m)
    ro, rd = frame_rays(g, cuda)
    ro, rd = ro[:, :n].contiguous(), rd[:, :n].contiguous()
    kw = dict(dt_gamma=float(g["dt_gamma"]), **gui(kind, False), **KW)
    r = frame(c, ro, rd, **kw)
    identical(r, frame(m, ro, rd, **kw), keys_of(kind), n)
    close(r["image"].view(-1, 3), g["image"].reshape(-1, 3)[:n], what="image")      # the first rays of the golden frame
    assert c.reached == 0


# ---------------------------------------------------------------- 3. the model as it is at the call
def _sparse_bits(x):
    x.density_bitfield = raymarching.packbits(torch.from_numpy(scene.sparse_density_grid(fill=0.5)).to(x.density_bitfield.device), 0.5)


def _set_edit(x):
    set_extra_edit(x, x.opt, x.basis_color.device)


def _palette_settings(x):
    with torch.no_grad():
        x.basis_color.mul_(0.5).add_(0.1)
    x.offsets_weight, x.view_dep_weight = 0.25, 0.5


def _data_writes(x):      # behind torch's version counters, as torch_ema's copy_to / restore write (palette/utils.py:782-784)
    x.color_net[1].weight.data.mul_(-1.0)
    x.encoder.embeddings.data[:60000].mul_(-0.5)


def _scalars(x):
    x.density_scale, x.min_near = 7.0, 0.5
    x.aabb_infer = x.aabb_infer * 0.75


def _clear_edit(x):
    x.edit = None


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_every_frame_sees_the_model_as_it_is(cuda, kind):
    """The GUI and the Trainer of the reference mutate the model between frames.  After each change the caller's next frame equals, bit for bit, the
    frame of a freshly built mirror model that was given the same changes."""
    changes = ([_palette_settings] if kind == "palette" else []) + [_data_writes, _sparse_bits, _scalars] + ([_set_edit, _clear_edit] if kind == "palette" else [])
    build = lambda: mirror(kind, cuda, seed=2, density_scale=25.0)
    c = caller_of(build())
    ro, rd = rays(cuda, 40, 36)
    kw = dict(**gui(kind, False), **KW)
    last = frame(c, ro, rd, **kw)
    identical(last, frame(build(), ro, rd, **kw), keys_of(kind), "unchanged")
    for i, change in enumerate(changes):
        change(c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # a `.data` write is noticed by the frame's source checksums: rebuilt, rendered again, and said so
            r = frame(c, ro, rd, **kw)
        fresh = build()
        for earlier in changes[:i + 1]:
            earlier(fresh)
        identical(r, frame(fresh, ro, rd, **kw), keys_of(kind), change.__name__)
        if change is not _clear_edit:
            assert not torch.equal(torch.nan_to_num(r["image"]), torch.nan_to_num(last["image"])), change.__name__      # the change did reach the frame
        last = r
    assert c.reached == 0


def test_results_belong_to_the_caller(cuda):
    m = mirror("palette", cuda, seed=4, density_scale=25.0, pred_clip=True)
    c = caller_of(m)
    a = frame(c, *rays(cuda, 40, 36, azimuth=45.0), gui_mode=True, **KW)
    kept = {k: a[k].clone() for k in ("image", "depth", "clip_feat")}
    b = frame(c, *rays(cuda, 40, 36, azimuth=160.0), gui_mode=True, **KW)
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(v)), k
        assert not torch.equal(torch.nan_to_num(b[k]), torch.nan_to_num(v)), k
    assert float(a["clip_feat"].abs().max()) > 0 and c.reached == 0


# ---------------------------------------------------------------- 4. what is no inference frame, and the mirror class itself
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_training_and_autograd_calls_reach_the_class_method_on_the_device(cuda, kind):
    c = caller_of(mirror(kind, cuda, seed=1, density_scale=20.0))
    ro, rd = rays(cuda, 8, 8)
    c.train()
    with pytest.raises(Reached), torch.no_grad():
        c.run_cuda(ro, rd, **KW)
    c.eval()
    with pytest.raises(Reached), torch.enable_grad():
        c.run_cuda(ro, rd, **KW)
    with pytest.raises(Reached), torch.no_grad():
        c.run_cuda(ro.double(), rd.double(), **KW)
    assert c.reached == 3
    assert "iterations" in frame(c, ro, rd, **KW) and c.reached == 3
    dropin.unfuse(c)
    with pytest.raises(Reached), torch.no_grad():
        c.run_cuda(ro, rd, **KW)


@pytest.mark.parametrize("order", ["loop_first", "field_first"])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_mirror_class_with_fuse_loop_and_fuse_field(cuda, kind, order):
    """On this package's own class, left in its default per-op mode: fuse_loop alone decides that inference frames take the frame call, in either
    order with fuse_field; a training-mode call still runs the class's own (differentiable) path."""
    want = frame(mirror(kind, cuda, seed=6, density_scale=20.0), *rays(cuda, 24, 20), **gui(kind, False), **KW)
    m = mirror(kind, cuda, seed=6, density_scale=20.0)
    m.march_mode, m.fused_field = "compat", False
    steps = [dropin.fuse_loop, dropin.fuse_field]
    for step in (steps if order == "loop_first" else steps[::-1]):
        step(m)
    ro, rd = rays(cuda, 24, 20)
    with torch.no_grad():
        r = m.render(ro, rd, **gui(kind, False), **KW)
    identical(r, want, keys_of(kind), order)
    if kind == "nerf":
        m.train()
        t = m.run_cuda(ro, rd, perturb=False, force_all_rays=True)
        assert t["image"].requires_grad and "iterations" not in t
