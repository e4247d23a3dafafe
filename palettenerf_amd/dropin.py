"""Register the operator modules under the import names the reference's callers use, so that
nerf/renderer.py, palette/renderer.py, nerf/network.py, palette/network.py and encoding.py run
unchanged on MI355X:

    import palettenerf_amd.dropin as dropin; dropin.install()
    import raymarching                      # -> palettenerf_amd.raymarching
    from gridencoder import GridEncoder     # -> palettenerf_amd.gridencoder.GridEncoder
    from shencoder import SHEncoder         # -> palettenerf_amd.shencoder.SHEncoder
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
    (pnr_background_forward over the coordinates the caller's sph_from_ray produced) for the same inference batches, the model's own method otherwise;
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


def bind_background(model):
    """fuse_field's background half: `model.background` as an instance attribute over the model's own BackgroundFused (pipeline.clone_for_concurrent_frames
    binds a twin's again, over the twin's).  Nothing is bound without a background or for an architecture the launch does not support: the per-op
    formulation stays."""
    import torch
    from .fused import background_fused
    model.__dict__.pop("background", None)
    bg_fused = background_fused(model) if getattr(model, "bg_radius", 0) > 0 and getattr(model, "bg_net", None) is not None else None
    if bg_fused is None:
        return
    plain_bg = model.background

    def background(x, d):
        if torch.is_grad_enabled() or torch.is_autocast_enabled() or not x.is_cuda:
            return plain_bg(x, d)
        return bg_fused.from_coords(x, d)

    model.background = background
