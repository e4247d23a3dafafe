"""Register the operator modules under the import names the reference's callers use, so that
nerf/renderer.py, palette/renderer.py, nerf/network.py, palette/network.py and encoding.py run
unchanged on MI355X:

    import palettenerf_amd.dropin as dropin; dropin.install()
    import raymarching                      # -> palettenerf_amd.raymarching
    from gridencoder import GridEncoder     # -> palettenerf_amd.gridencoder.GridEncoder
    from shencoder import SHEncoder         # -> palettenerf_amd.shencoder.SHEncoder

Two opt-in steps beyond the operator boundary, each bound on ONE model instance (no class and no reference file is touched):
fuse_field(model) -- forward() on the fused field kernel; fuse_loop(model) -- run_cuda() on the device-driven frame loop; unfuse(model) removes both.
"""
import sys
import types

from . import gridencoder as _ge
from . import palette_utils as _pu
from . import raymarching as _rm
from . import shencoder as _sh


def _package(name, module, submodule_name):
    pkg = types.ModuleType(name)
    pkg.__path__ = []  # mark as package so `import name.sub` works
    for k, v in vars(module).items():
        if not k.startswith("__"):
            setattr(pkg, k, v)
    setattr(pkg, submodule_name, module)
    sys.modules[name] = pkg
    sys.modules[f"{name}.{submodule_name}"] = module
    return pkg


def install(patch_palette_utils=True):
    """Idempotent.  Returns the dict of installed module names."""
    installed = {
        "raymarching": _package("raymarching", _rm, "raymarching"),         # raymarching/raymarching.py
        "gridencoder": _package("gridencoder", _ge, "grid"),                # gridencoder/grid.py
        "shencoder": _package("shencoder", _sh, "sphere_harmonics"),        # shencoder/sphere_harmonics.py
    }
    if patch_palette_utils and "palette.utils" in sys.modules:
        # palette/utils.py is mostly harness code; only its two HSV operators are native (palette/utils.py:257-295)
        pu = sys.modules["palette.utils"]
        pu.rgb_to_hsv, pu.hsv_to_rgb = _pu.rgb_to_hsv, _pu.hsv_to_rgb
    return installed


def fuse_field(model, precision="f16x3", pair_lookup=False):
    """Opt-in, one step beyond the operator boundary: give a NeRFNetwork or PaletteNetwork -- the REFERENCE's own class (nerf/network.py, built over the drop-in
    encoders after install()) or this package's mirror -- the fused MFMA field kernel as its forward() for inference batches.  The reference's
    renderer (`run_cuda`'s while loop, its boolean-mask compaction, its composite_rays calls) and its network file stay unchanged; what
    changes is what `self(xyzs, dirs)` executes: one hash-grid lookup + ONE fused launch (sigma_net, SH, color_net, exp / sigmoid on the
    matrix cores, pnr_nerf_field_forward) instead of encoder permute-copy + 5 GEMMs + 6 elementwise launches.  Same (sigma, rgb) to 2e-6
    (tests/test_gpu_ops.py), images to 1e-4 of the reference-driven goldens (tests/test_gpu_frames.py).  Batches under autograd or autocast, and
    CPU tensors, keep the model's own forward.  The model must have the shipped architecture (hashgrid 16 x 2, 64-wide nets, SH degree 4);
    NeRFFieldFused raises otherwise.  precision: "f16x3" (split-fp16 products, fp32-class), "fp32" (exact fmaf chains) or "f16x2" (opt-in).
    pair_lookup (PaletteNetwork only): look both hash tables up through one interleaved copy (PaletteFieldFused.stand_alone_pair).  The copy follows torch's
    version counters only: after writing the tables through `.data` (torch_ema's copy_to / restore around an evaluation) call
    invalidate_fused_caches(model), or the forward reads the old tables.  Default: the live tables, whatever wrote them.
    A model with a background (bg_radius > 0) also gets `background(x, d)` bound the same way: encoder_bg, SH, bg_net and the sigmoid as one launch
    (pnr_background_forward over the coordinates the caller's sph_from_ray produced) for the same inference batches, one launch each way for training
    batches (fp32 device inputs that need no gradient; pnr_background_train_forward / pnr_background_backward, `model.fused_train_background = False` turns
    that off), the model's own method otherwise;
    a background that is not the reference's architecture (4 x 2 levels, SH degree 4, 24 -> 64 -> 3) keeps the model's own method."""
    import torch
    from .fused import NeRFFieldFused, PaletteFieldFused
    plain = model.forward
    if hasattr(model, "encoder_palette"):
        # PaletteNetwork (palette/network.py): forward(x, d) -> (sigma, clip_feat, omega, offsets_radiance, view_dep, diffuse) from two (three) lookups +
        # ONE fused launch (12-14 layers, SH, ELU, the heads' softplus normalisation; pnr_palette_field_forward with the network-heads row).  The
        # colour-basis composite and RegionEdit / Stylizer stay the reference renderer's own code; its seven composite_rays_flex calls stay where they are and reach
        # the device as one launch (below).
        fused = PaletteFieldFused(model)
        fused.precision = {"fp32": 0, "f16x3": 1, "f16x2": 1}[precision]
        fused.stand_alone_pair = bool(pair_lookup)

        def run(x, d):
            out = fused.network_forward(x, d)
            # what follows an inference forward() in run_cuda are the iteration's six / seven composite_rays_flex calls and then composite_rays
            # (palette/renderer.py:508-519): they are collected and issued as ONE pnr_composite_rays_flex_multi launch in front of that composite_rays
            # (raymarching._FlexQueue: same bits; the deferral ends with that call, and arms only inside a march iteration, for its rays)
            _rm.arm_flex_deferral_in_iteration()
            return out
    else:
        fused = NeRFFieldFused(model)
        fused.precision = {"fp32": 0, "f16x3": 1, "f16x2": 2}[precision]
        run = fused.__call__

    def forward(x, d):
        if torch.is_grad_enabled() or torch.is_autocast_enabled() or not x.is_cuda:
            return plain(x, d)
        return run(x, d)

    model._fused = fused
    model.forward = forward      # instance attribute: nn.Module.__call__ resolves self.forward here
    bind_background(model)
    return model


_LOOP_PRECISION = {"fp32": 0, "f16x3": 1, "f16x2": 2}


class _Loop:
    """What fuse_loop keeps on the instance (`model._loop`): the precision it was asked for and the all-zero maps the frames hand out
    (renderer._zero_map).  The field object itself is `model._fused`, shared with fuse_field and looked up per frame."""

    def __init__(self, precision):
        self.precision = precision


def fuse_loop(model, precision="f16x3"):
    """Opt-in, one step beyond fuse_field: give a NeRFNetwork or PaletteNetwork -- the REFERENCE's own class (built over the drop-in encoders after
    install()) or this package's mirror -- the device-driven frame loop as its run_cuda() for inference frames.  The reference's renderer file stays
    unchanged; what changes is what `model.run_cuda(rays_o, rays_d, ...)` (and so `model.render`) executes for a frame: instead of the while loop of
    nerf/renderer.py:336-386 / palette/renderer.py:430-550 -- march_rays, forward, six flex composites, composite_rays and a boolean-mask compaction
    with its host sync per iteration -- ONE call of pnr_nerf_render_frame / pnr_palette_render_frame (fused._FrameLoop.render_frame), which also
    computes near / far, the background blend and the depth normalisation.  Same signature, unknown keywords ignored, the reference's result keys
    with its shapes in fp32 (plus the mirror's n_samples / rendered / iterations ...); every tensor is the caller's to keep.

    A call takes the native frame when model.cuda_ray is set, the model is in eval mode, autograd is off and the rays are fp32 on the model's HIP
    device; under fp16 autocast (-O) the frame reads half tables, perturb draws the one torch.rand(N) the per-op loop draws (or takes `noises=`),
    bg_radius > 0 costs one launch (the model's own background() when its architecture is not the reference's), model.edit and -- in gui_mode --
    model.stylizer run in the field kernel's epilogue.  Every other call (training, autograd on, CPU tensors, the Stylizer outside gui_mode) goes to
    the class's own run_cuda, untouched.  The model is read as it is at each call: bitfield, aabb, scalars, palette, edit state, every weight and
    table -- writes through `.data` included (torch_ema's copy_to / restore): the frame's source checksums notice them, rebuild the packed blobs and
    render the frame again (a warning says so; invalidate_fused_caches(model) after such a write avoids the double render; a write to only PART of a
    table needs it, see fused._SourceWatch).
    The model must have the shipped architecture (hashgrid 16 x 2, 64-wide nets, SH degree 4): RuntimeError here otherwise.  precision as fuse_field's
    ("f16x2" is honoured where the frame kernels have that form).  Composes with fuse_field in either order; unfuse(model) removes both."""
    import torch
    from . import renderer as _rd
    from .fused import NeRFFieldFused, PaletteFieldFused, background_fused
    palette = hasattr(model, "encoder_palette")
    make = PaletteFieldFused if palette else NeRFFieldFused
    if precision not in _LOOP_PRECISION:
        raise ValueError(f"precision must be one of {sorted(_LOOP_PRECISION)}")
    if model.__dict__.get("_fused") is None:
        model._fused = make(model)       # (raises for another architecture; one that is there already has passed this check)
    loop = model._loop = _Loop(_LOOP_PRECISION[precision])

    def native(rays_o, rays_d, kwargs):
        """The frame can go to the frame call as far as the rays and the model's mode say."""
        return (bool(model.cuda_ray) and not model.training and not torch.is_grad_enabled() and rays_o.is_cuda and rays_o.dtype == torch.float32
                and rays_d.dtype == torch.float32 and rays_d.device == rays_o.device and rays_o.shape == rays_d.shape and rays_o.numel() > 0
                and model.aabb_infer.device == rays_o.device and kwargs.get("_phase") is None)

    def field():
        fused = model.__dict__.get("_fused")
        if fused is None:               # (invalidated by hand: `model._fused = None`)
            fused = model._fused = make(model)
        return fused

    def frame(fused, call):
        was = fused.precision
        fused.precision = loop.precision
        try:
            return call()
        finally:
            fused.precision = was

    def flat_rays(rays_o, rays_d):
        return rays_o.shape[:-1], rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3)

    def bg_of(rays_o, rays_d, bg_color):
        if model.bg_radius > 0:         # nerf/renderer.py:274-277: one launch, or the model's own background() as the frame's bg_map
            bg = background_fused(model)
            if bg is not None:
                return bg.from_rays(rays_o, rays_d)
            return model.background(_rm.sph_from_ray(rays_o, rays_d, model.bg_radius), rays_d)
        return 1 if bg_color is None else bg_color

    if palette:
        def run_cuda(rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-4, gui_mode=False, **kwargs):
            if not native(rays_o, rays_d, kwargs) or (model.stylizer is not None and not gui_mode):
                return type(model).run_cuda(model, rays_o, rays_d, dt_gamma=dt_gamma, bg_color=bg_color, perturb=perturb, force_all_rays=force_all_rays,
                                            max_steps=max_steps, T_thresh=T_thresh, gui_mode=gui_mode, **kwargs)
            prefix, rays_o, rays_d = flat_rays(rays_o, rays_d)
            bg_color = bg_of(rays_o, rays_d, bg_color)
            noises = _rd._frame_noises(perturb, kwargs.get("noises"), rays_o.shape[0], rays_o)
            fused = field()
            return frame(fused, lambda: _rd.palette_native_frame(model, fused, loop, rays_o, rays_d, prefix, model.aabb_infer, None, None, bg_color, noises,
                                                                 dt_gamma, max_steps, T_thresh, gui_mode))
    else:
        def run_cuda(rays_o, rays_d, rays_gt=None, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-4, **kwargs):
            if not native(rays_o, rays_d, kwargs):
                return type(model).run_cuda(model, rays_o, rays_d, rays_gt=rays_gt, dt_gamma=dt_gamma, bg_color=bg_color, perturb=perturb,
                                            force_all_rays=force_all_rays, max_steps=max_steps, T_thresh=T_thresh, **kwargs)
            prefix, rays_o, rays_d = flat_rays(rays_o, rays_d)
            bg_color = bg_of(rays_o, rays_d, bg_color)
            noises = _rd._frame_noises(perturb, kwargs.get("noises"), rays_o.shape[0], rays_o)
            fused = field()
            return frame(fused, lambda: _rd.nerf_native_frame(model, fused, loop, rays_o, rays_d, prefix, model.aabb_infer, None, None, bg_color, noises,
                                                              dt_gamma, max_steps, T_thresh))

    model.run_cuda = run_cuda    # instance attribute: render() and the Trainer resolve self.run_cuda here; type(model).run_cuda stays what it was
    return model


def unfuse(model):
    """Remove what fuse_loop and fuse_field bound: run_cuda, forward and background are the class's methods again, and the fused objects (with their
    packed blobs, table copies and workspaces) are dropped."""
    for name in ("run_cuda", "forward", "background", "_loop"):
        model.__dict__.pop(name, None)
    from .renderer import _RendererBase
    for name in ("_fused", "_bg_fused"):
        if name in model.__dict__:
            if isinstance(model, _RendererBase):    # the mirror's constructors define both (None until first use)
                model.__dict__[name] = None
            else:
                del model.__dict__[name]
    return model


def bind_background(model):
    """fuse_field's background half: `model.background` as an instance attribute over the model's own BackgroundFused (pipeline.clone_for_concurrent_frames
    binds a twin's again, over the twin's).  Nothing is bound without a background or for an architecture the launch does not support: the per-op
    formulation stays."""
    import torch
    from .fused import background_fused, background_train_fused
    model.__dict__.pop("background", None)
    bg_fused = background_fused(model) if getattr(model, "bg_radius", 0) > 0 and getattr(model, "bg_net", None) is not None else None
    if bg_fused is None:
        return
    plain_bg = model.background

    def background(x, d):
        if torch.is_grad_enabled():       # training batches: one launch each way, unless model.fused_train_background says no
            train = background_train_fused(model, x, d, fused_kernels=True)     # the model's BackgroundFused as it is NOW, or None
            return train.train_from_coords(x, d) if train is not None else plain_bg(x, d)
        if torch.is_autocast_enabled() or not x.is_cuda:
            return plain_bg(x, d)
        return bg_fused.from_coords(x, d)

    model.background = background
