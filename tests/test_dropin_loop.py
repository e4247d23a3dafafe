"""dropin.fuse_loop / dropin.unfuse on the host side (no GPU): what is bound where, which calls fall through to the class's own run_cuda, what
unfuse leaves behind -- on this package's mirror classes and, where the reference tree is present, on the reference's own NeRFNetwork /
PaletteNetwork built over the drop-in encoders.  The frames themselves: tests/test_gpu_dropin_loop.py."""
import inspect
import os
import sys
import types

import pytest
import torch

from palettenerf_amd import dropin, pipeline, renderer
import palettenerf_amd.network as mine

REF = os.environ.get("PNR_REFERENCE_DIR", "/root/reference")

# nerf/renderer.py:258 and palette/renderer.py:296-297
NERF_SIGNATURE = ["rays_o", "rays_d", "rays_gt", "dt_gamma", "bg_color", "perturb", "force_all_rays", "max_steps", "T_thresh", "kwargs"]
PALETTE_SIGNATURE = ["rays_o", "rays_d", "dt_gamma", "bg_color", "perturb", "force_all_rays", "max_steps", "T_thresh", "gui_mode", "kwargs"]


def recording(cls):
    """A throw-away subclass whose class-level run_cuda records its call instead of rendering."""
    calls = []

    class Recording(cls):
        def run_cuda(self, rays_o, rays_d, **kwargs):
            calls.append((self, rays_o, rays_d, kwargs))
            return "the class's own run_cuda"

    return Recording, calls


def mirror(kind, cls=None, **kw):
    if kind == "nerf":
        return (cls or mine.NeRFNetwork)(bound=2, cuda_ray=True, **kw)
    return (cls or mine.PaletteNetwork)(renderer.default_opt(), bound=2, cuda_ray=True, **kw)


def falls_through(m, calls, kind):
    """CPU rays, training mode and autograd each send the call to the class's method, with every argument -- unknown keywords too -- as given."""
    ro, rd = torch.zeros(1, 5, 3), torch.ones(1, 5, 3)
    extra = dict(workspace="trial", fp16=True, num_steps=512)      # the reference's callers pass **vars(opt)
    m.eval()
    with torch.no_grad():
        assert m.run_cuda(ro, rd, dt_gamma=0.25, perturb=True, **extra) == "the class's own run_cuda"
        assert m.render(ro, rd, staged=True, bg_color=0.5) == "the class's own run_cuda"
    m.train()
    with torch.no_grad():
        m.run_cuda(ro, rd, **extra)
    m.eval()
    with torch.enable_grad():
        m.run_cuda(ro, rd, **extra)
    assert len(calls) == 4 and all(c[0] is m and c[1] is ro and c[2] is rd for c in calls)
    first = calls[0][3]
    assert first["dt_gamma"] == 0.25 and first["perturb"] is True and first["max_steps"] == 1024 and first["T_thresh"] == 1e-4
    assert all(first[k] == v for k, v in extra.items())
    assert calls[1][3]["bg_color"] == 0.5
    assert ("gui_mode" in first) == (kind == "palette") and ("rays_gt" in first) == (kind == "nerf")
    del calls[:]


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_fuse_loop_binds_run_cuda_on_the_instance_and_unfuse_takes_it_off(kind):
    m = mirror(kind)
    before = dict(m.__dict__)
    class_run_cuda, class_forward = type(m).run_cuda, type(m).forward
    assert dropin.fuse_loop(m) is m
    assert "run_cuda" in m.__dict__ and type(m).run_cuda is class_run_cuda and "forward" not in m.__dict__
    assert list(inspect.signature(m.run_cuda).parameters) == (NERF_SIGNATURE if kind == "nerf" else PALETTE_SIGNATURE)
    assert inspect.signature(m.run_cuda).parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    new = set(m.__dict__) - set(before)
    assert new == {"run_cuda", "_loop"}, new                      # one private attribute next to _fused
    assert m._fused is not None and m._fused.model is m
    dropin.fuse_field(m)
    assert "forward" in m.__dict__ and type(m).forward is class_forward
    assert dropin.unfuse(m) is m
    assert set(m.__dict__) == set(before) and all(m.__dict__[k] is v for k, v in before.items())
    assert m.run_cuda.__func__ is class_run_cuda and m.forward.__func__ is class_forward
    dropin.unfuse(m)                                               # nothing bound: nothing to do


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_calls_that_are_no_inference_frames_on_the_device_reach_the_class_method(kind):
    cls, calls = recording(mine.NeRFNetwork if kind == "nerf" else mine.PaletteNetwork)
    m = dropin.fuse_loop(mirror(kind, cls))
    falls_through(m, calls, kind)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_another_architecture_is_refused_at_bind_time(kind):
    m = mirror(kind, hidden_dim=32)
    with pytest.raises(RuntimeError, match="specialised for the shipped architecture"):
        dropin.fuse_loop(m)
    assert "run_cuda" not in m.__dict__ and "_loop" not in m.__dict__
    with pytest.raises(ValueError):
        dropin.fuse_loop(mirror(kind), precision="fp8")


@pytest.mark.parametrize("order", ["loop_first", "field_first"])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_fuse_loop_composes_with_fuse_field_in_either_order(kind, order):
    cls, calls = recording(mine.NeRFNetwork if kind == "nerf" else mine.PaletteNetwork)
    m = mirror(kind, cls)
    steps = [dropin.fuse_loop, dropin.fuse_field]
    for step in (steps if order == "loop_first" else steps[::-1]):
        assert step(m, precision="fp32") is m
    assert "run_cuda" in m.__dict__ and "forward" in m.__dict__
    assert m._fused.precision == 0 and m._loop.precision == 0
    falls_through(m, calls, kind)                                  # (what falls through then runs the fused forward: self(xyzs, dirs) resolves on the instance)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_a_twin_for_concurrent_frames_gets_its_own_binding(kind):
    m = dropin.fuse_loop(mirror(kind), precision="fp32")
    twin = pipeline.clone_for_concurrent_frames(m)
    assert twin.__dict__["run_cuda"] is not m.__dict__["run_cuda"] and twin._loop is not m._loop and twin._fused is not m._fused
    assert twin._fused.model is twin and twin._loop.precision == 0
    own = twin.__dict__["run_cuda"], twin._loop
    m._loop.precision = 1
    pipeline.sync_twin(m, twin)
    assert (twin.__dict__["run_cuda"], twin._loop) == own and twin._loop.precision == 1


def _reference_classes():
    """The reference's nerf.network / palette.network imported over the drop-in operator modules (dropin.install()).  Its harness modules
    (nerf/utils.py, palette/utils.py: cv2, tensorboardX, lpips, ...) are replaced by the few functions the renderer and network files take from
    them; trimesh (imported for a debugging plot) by an empty module."""
    dropin.install()
    nu = types.ModuleType("nerf.utils")
    nu.custom_meshgrid = lambda *a: torch.meshgrid(*a, indexing="ij")
    nu.srgb_to_linear = lambda x: torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    from palettenerf_amd import palette_utils
    pu = types.ModuleType("palette.utils")
    pu.normalize = lambda t: t / (t.norm(dim=-1, keepdim=True) + 1e-9)
    pu.rgb_to_hsv, pu.hsv_to_rgb = palette_utils.rgb_to_hsv, palette_utils.hsv_to_rgb
    pal = types.ModuleType("palette")
    pal.__path__ = [os.path.join(REF, "palette")]
    pal.utils = pu
    sys.modules.update({"nerf.utils": nu, "palette": pal, "palette.utils": pu})
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    sys.path.insert(0, REF)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)     # torch.cuda.amp.custom_fwd, which the reference's activation.py uses, is deprecated
        import nerf.network as ref_nerf
        import palette.network as ref_palette
    assert ref_nerf.__file__.startswith(REF) and ref_palette.__file__.startswith(REF)
    return ref_nerf.NeRFNetwork, ref_palette.PaletteNetwork


@pytest.fixture
def reference_classes():
    if not os.path.isfile(os.path.join(REF, "nerf", "network.py")):
        pytest.skip("the reference tree is not on this machine")
    modules, path = dict(sys.modules), list(sys.path)
    try:
        yield _reference_classes()
    finally:
        sys.path[:] = path
        for name in [n for n in sys.modules if n not in modules]:
            del sys.modules[name]
        sys.modules.update(modules)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_fuse_loop_on_the_reference_classes(reference_classes, kind):
    """The REFERENCE's own NeRFNetwork / PaletteNetwork, constructed after dropin.install(): fuse_loop accepts the instance (it carries every
    attribute the frame path reads, and none of the mirror's), binds run_cuda on it alone, and sends what is no inference frame on the device to
    the reference's method."""
    from palettenerf_amd.gridencoder import GridEncoder
    ref_cls = reference_classes[0 if kind == "nerf" else 1]
    cls, calls = recording(ref_cls)
    m = cls(bound=2, cuda_ray=True) if kind == "nerf" else cls(renderer.default_opt(), bound=2, cuda_ray=True)
    assert not isinstance(m, renderer._RendererBase) and isinstance(m.encoder, GridEncoder)
    for name in ("march_mode", "fused_field", "_fused", "_bg_fused", "_native_frame", "_background_of_rays"):
        assert not hasattr(m, name), name
    m.eval()
    before = dict(m.__dict__)
    assert dropin.fuse_loop(m) is m and "run_cuda" in m.__dict__ and type(m).run_cuda is cls.run_cuda and ref_cls.run_cuda is not cls.run_cuda
    assert set(m.__dict__) - set(before) == {"run_cuda", "_loop", "_fused"}
    assert list(inspect.signature(m.run_cuda).parameters) == list(inspect.signature(ref_cls.run_cuda).parameters)[1:]
    assert [tuple(w.shape) for w in m._fused._weights()][:2] == [(64, 32), (16, 64)]
    falls_through(m, calls, kind)
    dropin.fuse_field(m)
    falls_through(m, calls, kind)
    dropin.unfuse(m)
    assert set(m.__dict__) == set(before) and all(m.__dict__[k] is v for k, v in before.items())
    wide = ref_cls(bound=2, cuda_ray=True, hidden_dim=32) if kind == "nerf" else ref_cls(renderer.default_opt(), bound=2, cuda_ray=True, hidden_dim=32)
    with pytest.raises(RuntimeError, match="specialised for the shipped architecture"):
        dropin.fuse_loop(wide)
