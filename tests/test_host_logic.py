"""CPU suite: this repo's renderer/network mirror (host logic), driven by the oracle facades instead
of the HIP operators, reproduces the golden frames produced by the reference's own Python callers."""
import os

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import network, renderer, scene
from oracle.facade import make_oracle_modules

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def install_facade(setattr_=setattr):
    """The oracle's facades in place of the mirror's kernel layer (`setattr_`: monkeypatch.setattr in a test, plain setattr in a child process)."""
    rm, ge, sh, pu = make_oracle_modules()
    import palettenerf_amd.gridencoder as pge
    import palettenerf_amd.shencoder as psh
    setattr_(renderer, "raymarching", rm)
    setattr_(renderer, "rgb_to_hsv", pu.rgb_to_hsv)
    setattr_(renderer, "hsv_to_rgb", pu.hsv_to_rgb)
    setattr_(pge, "GridEncoder", ge.GridEncoder)
    setattr_(psh, "SHEncoder", sh.SHEncoder)
    return rm


@pytest.fixture()
def facade(monkeypatch):
    return install_facade(monkeypatch.setattr)


def rays(g):
    H, W = int(g["H"]), int(g["W"])
    pose = torch.from_numpy(scene.lookat_pose())[None]
    return scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)


def put_scene(m):
    grid = scene.brick_density_grid()
    m.density_grid.copy_(torch.from_numpy(grid))
    m.density_bitfield.copy_(torch.from_numpy(oracle.packbits(grid, 0.5)))


@pytest.mark.parametrize("case", ["a", "b"])
def test_nerf_mirror_reproduces_reference_frames(facade, case):
    g = np.load(os.path.join(GOLDEN, f"frame_nerf_{case}.npz"))
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=float(g["density_scale"]), min_near=0.2)
    scene.seed_field_(m, int(g["seed"]))
    put_scene(m)
    m.eval()
    ro, rd = rays(g)
    with torch.no_grad():
        r = m.render(ro, rd, staged=True, dt_gamma=float(g["dt_gamma"]), perturb=False, max_steps=1024, T_thresh=1e-4)
    for k in ("image", "depth", "weights_sum"):
        np.testing.assert_allclose(r[k].numpy(), g[k], rtol=0, atol=1e-6, err_msg=k)
    gt = np.load(os.path.join(GOLDEN, f"train_nerf_{case}.npz"))
    m.train()
    r = m.run_cuda(ro, rd, dt_gamma=float(gt["dt_gamma"]), perturb=False, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
    assert m.step_counter[0].numpy().tolist() == gt["counter"].tolist()
    np.testing.assert_allclose(r["image"].detach().numpy(), gt["image"], atol=1e-6)


def test_palette_mirror_reproduces_reference_frames(facade):
    g = np.load(os.path.join(GOLDEN, "frame_palette_a.npz"))
    opt = renderer.default_opt(pred_clip=bool(g["pred_clip"]))
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=float(g["density_scale"]), min_near=0.2)
    scene.seed_field_(m, int(g["seed"]))
    put_scene(m)
    m.eval()
    ro, rd = rays(g)
    with torch.no_grad():
        r = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=False)
    for k in ("image", "depth", "depth_origin", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
        np.testing.assert_allclose(r[k].numpy(), g[k], rtol=0, atol=1e-6, err_msg=k)
    m.edit = renderer.RegionEdit(opt)
    m.edit.update_cent(mean_xyz=torch.tensor([0.1, 0.0, -0.2]))
    m.edit.update_std(std_xyz=0.5)
    m.edit.update_delta_hsv(m.basis_color.data.clamp(0, 1), (m.basis_color.data * 0.6 + 0.2).flip(0).clamp(0, 1))
    with torch.no_grad():
        r2 = m.render(ro, rd, dt_gamma=float(g["dt_gamma"]), perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=True)
    np.testing.assert_allclose(r2["image"].numpy(), g["edit_image"], atol=1e-6)


def _extra_model(g):
    opt = renderer.default_opt(pred_clip=bool(g["pred_clip"]), num_basis=int(g["num_basis"]))
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=float(g["density_scale"]), min_near=0.2)
    scene.seed_field_(m, int(g["seed"]))
    return opt, m


def set_extra_edit(m, opt, device="cpu"):
    """The RegionEdit state of the `frame_palette_{style,nb}*` fixtures (tests/golden/gen_golden.py:gen_palette_extra)."""
    m.edit = renderer.RegionEdit(opt)
    m.edit.update_cent(mean_xyz=torch.tensor([0.1, 0.0, -0.2], device=device), mean_clip=torch.linspace(-0.3, 0.3, 16).to(device))
    m.edit.update_std(std_xyz=0.5, std_clip=2.0)
    m.edit.update_delta_hsv(m.basis_color.data.clamp(0, 1), (m.basis_color.data * 0.6 + 0.2).flip(0).clamp(0, 1))


def set_extra_stylizer(m, opt, g, device="cpu"):
    m.stylizer = renderer.Stylizer(opt).to(device)
    with torch.no_grad():
        for k, v in scene.stylizer_state(int(g["num_basis"]), int(g["seed"])).items():
            getattr(m.stylizer, k).copy_(v)


@pytest.mark.parametrize("case", ["style_a", "style_b", "nb6", "nb8"])
def test_palette_mirror_reproduces_stylizer_edit_and_many_basis_frames(facade, case):
    """Fixtures from the reference's own Stylizer / RegionEdit classes and PaletteNetwork with 4, 6 and 8 bases (gen_palette_extra)."""
    g = np.load(os.path.join(GOLDEN, f"frame_palette_{case}.npz"))
    opt, m = _extra_model(g)
    put_scene(m)
    m.eval()
    ro, rd = rays(g)
    kw = dict(dt_gamma=float(g["dt_gamma"]), perturb=False, max_steps=1024, T_thresh=1e-4)
    with torch.no_grad():
        r = m.render(ro, rd, gui_mode=False, **kw)
        for k in ("image", "depth", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
            np.testing.assert_allclose(r[k].numpy(), g[k], rtol=0, atol=1e-6, err_msg=k)
        set_extra_stylizer(m, opt, g)
        np.testing.assert_allclose(m.render(ro, rd, gui_mode=True, **kw)["image"].numpy(), g["style_image"], atol=1e-6)
        m.stylizer = None
        set_extra_edit(m, opt)
        e = m.render(ro, rd, gui_mode=False, **kw)
        np.testing.assert_allclose(e["image"].numpy(), g["edit_image"], atol=1e-6)
        np.testing.assert_allclose(e["basis_rgb"].numpy(), g["edit_basis_rgb"], atol=1e-6)
        m.edit.weight_mode = True
        np.testing.assert_allclose(m.render(ro, rd, gui_mode=True, **kw)["image"].numpy(), g["edit_weight_image"], atol=1e-6)


def test_state_dict_names_match_reference_checkpoint_layout():
    m = network.PaletteNetwork(renderer.default_opt(pred_clip=True), bound=2, cuda_ray=True)
    keys = set(m.state_dict())
    for k in ("encoder.embeddings", "encoder.offsets", "encoder_palette.embeddings", "encoder_clip.embeddings", "sigma_net.0.weight", "sigma_net.1.weight",
              "color_net.0.weight", "color_net.2.weight", "diff_net.0.weight", "basis_net.1.weight", "offsets_radiance_net.weight",
              "offsets_radiance_net.bias", "omega_net.0.weight", "clip_net.1.weight", "basis_color", "density_grid", "density_bitfield", "aabb_train",
              "aabb_infer", "step_counter"):
        assert k in keys, k
    assert m.density_bitfield.numel() == 2 * 128 ** 3 // 8 and m.cascade == 2 and tuple(m.step_counter.shape) == (16, 2)
    assert m.sigma_net[0].weight.shape == (64, 32) and m.basis_net[0].weight.shape == (64, 35) and m.offsets_radiance_net.weight.shape == (13, 15)
    names = {id(p) for grp in m.get_params(1e-2) for p in (grp["params"] if isinstance(grp["params"], (list, tuple)) else [grp["params"]] if torch.is_tensor(grp["params"]) else list(grp["params"]))}
    assert id(m.basis_net[0].weight) not in names  # reference quirk 8: basis_net is not optimised


def test_render_without_cuda_ray():
    """PaletteRenderer has no uniform-sampling path (palette/renderer.py:292-294 raises); NeRFRenderer dispatches to run(), whose HIP
    operators refuse CPU tensors loudly (no CPU fallback in the product path)."""
    p = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=False)
    with pytest.raises(ValueError):
        p.render(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    m = network.NeRFNetwork(bound=2, cuda_ray=False)
    with pytest.raises((RuntimeError, AssertionError)):
        m.render(torch.zeros(1, 4, 3), torch.ones(1, 4, 3))


# ------------------------------------------------------------------ exact lattice jump (csrc/lattice.hpp, compiled for the host)
def _lattice_lib(tmp_path_factory):
    import ctypes
    import subprocess
    out = tmp_path_factory.mktemp("lattice") / "liblattice_check.so"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "lattice_check.cpp")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out), src])
    lib = ctypes.CDLL(str(out))
    lib.lattice_fuzz.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.lattice_case.argtypes = [ctypes.c_float] * 3 + [ctypes.c_void_p] * 4
    lib.lattice_steps_fuzz.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def test_lattice_steps_equals_k_plain_additions(tmp_path_factory):
    """lattice_steps(t, d, k) -- the k-th lattice point after t, which the wave-cooperative march tail hands to lane k -- must be bit for bit
    what k additions `t += d` give (raymarching.cu:389, :399-401)."""
    lib = _lattice_lib(tmp_path_factory)
    bad = np.zeros(3, np.float32)
    for mode in (0, 1, 2):
        for seed in (1, 2, 3):
            n = lib.lattice_steps_fuzz(seed * 104729 + mode, 200000, mode, bad.ctypes.data)
            assert n == 0, f"mode {mode} seed {seed}: {n} mismatches, first at (tc, d, k) = {bad}"


def test_lattice_advance_equals_the_stepping_loop(tmp_path_factory):
    """lattice_advance() must return bit-for-bit what `do { t += d } while (t < tt)` returns (raymarching.cu:399-401):
    generic steps, the steps the shipped configs produce, and steps with few mantissa bits (exact rounding ties)."""
    lib = _lattice_lib(tmp_path_factory)
    bad = np.zeros(3, np.float32)
    for mode in (0, 1, 2):
        for seed in (1, 2, 3):
            n = lib.lattice_fuzz(seed * 7919 + mode, 200000, mode, bad.ctypes.data)
            assert n == 0, f"mode {mode} seed {seed}: {n} mismatches, first at (tc, d, tt) = {bad}"
    # hand-picked: binade crossings landing exactly on a power of two, a target equal to the start, a NaN target
    out = [np.zeros(1, np.float32) for _ in range(4)]
    ptrs = [o.ctypes.data for o in out]
    for tc, d, tt in [(0.5, 0.25, 4.0), (1.0, 2.0 ** -23, 1.0 + 2.0 ** -20), (3.999999, 0.003382, 4.1), (1.5, 0.003382, 1.5),
                      (1.5, 0.003382, float("nan")), (0.2, 0.0270632, 7.9), (2.0 ** -130, 0.01, 0.5)]:
        assert lib.lattice_case(tc, d, tt, *ptrs) == 1, (tc, d, tt, [float(o[0]) for o in out])


# ------------------------------------------------------------------ the frame call's host arithmetic (csrc/frame_plan.hpp, compiled for the host)
def test_frame_plan_rules_equal_the_expressions_they_replaced(tmp_path):
    """tests/native/frame_plan_check.cpp: chunk lengths, row bounds, launch sizes and the march cap of csrc/frame_plan.hpp against a transcription of the
    expressions the frame driver held inline, exhaustively over the ranges listed there; a stand-alone program under the address and undefined-behaviour
    sanitizers (its own process, nothing preloaded).  Exit status 0 = every case agrees."""
    import subprocess
    exe = tmp_path / "frame_plan_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "frame_plan_check.cpp")
    subprocess.check_call(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", str(exe), src])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr


def test_option_table_equals_the_chain_and_initialisers_it_replaced(tmp_path):
    """tests/native/options_check.cpp: csrc/options.hpp (the table of options.def) against a transcription of pnr_set_option's chain of comparisons and of
    the getenv initialisers it replaced: return code and stored value for every name (an unknown one and NULL too) over [-3, 1100], INT_MIN, INT_MAX and
    65536; the starting values under every environment variable, alone and set to "", "0", "1", "2", "7", "5000", "-1", and under both of
    composite_fusion's together (a stand-in lookup, not the process environment); distinct names, and the per-frame options being the twelve that pnr.h
    lists at pnr_*_render_frame_submit.  A stand-alone program under the address and undefined-behaviour sanitizers, as above."""
    import subprocess
    exe = tmp_path / "options_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "options_check.cpp")
    subprocess.check_call(["g++", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", str(exe), src])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr


def test_frame_workspace_sizes_are_pinned():
    """The frame workspace's layout (frame.hip: carve) is part of what callers allocate: its totals for a few frame sizes and model shapes, as literals."""
    import ctypes
    from palettenerf_amd import _lib
    lib = _lib.load()
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    sizes = (0, 1, 255, 256, 257, 12288)
    assert [lib.pnr_nerf_frame_workspace_bytes(u32(n)) for n in sizes] == [40448, 40448, 105728, 105728, 110336, 3390720]
    want = {(4, 0, 0): [42240, 42240, 213248, 213248, 218624, 8503552],
            (8, 0, 0): [42240, 42240, 270080, 270592, 275968, 11256064],
            (4, 16, 1): [42496, 42496, 278784, 278784, 284416, 11649280]}
    for (nb, clip_dim, pred_clip), totals in want.items():
        assert [lib.pnr_palette_frame_workspace_bytes(u32(n), u32(nb), u32(clip_dim), i32(pred_clip)) for n in sizes] == totals, (nb, clip_dim, pred_clip)


# ------------------------------------------------------------------ f3: the reference's checkpoint files
def _layout():
    import json
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_dict_layout.json")))


def test_state_dict_layout_equals_the_reference_models():
    """Names, shapes and dtypes of both models' state_dict against the layout dumped from the reference's own modules
    (tests/golden/gen_golden.py layout): what makes its .pth files loadable here."""
    lay = _layout()
    n = network.NeRFNetwork(bound=2, cuda_ray=True)
    opt = renderer.default_opt()
    opt.pred_clip = True
    p = network.PaletteNetwork(opt, bound=2, cuda_ray=True)
    for name, m in (("nerf", n), ("palette", p)):
        mine = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
        assert mine == lay[name], (name, set(mine) ^ set(lay[name]))


def test_checkpoint_round_trip_in_the_reference_format(tmp_path):
    from palettenerf_amd import checkpoint
    src = network.NeRFNetwork(bound=2, cuda_ray=True)
    scene.seed_field_(src, 3)
    src.mean_count, src.mean_density = 4321, 0.125
    src.density_grid.uniform_(0, 2)
    src.density_bitfield.copy_(torch.from_numpy(oracle.packbits(src.density_grid.numpy(), 0.5)))
    # a trainer checkpoint as Trainer.save_checkpoint writes it (utils.py:1083-1143), the 'best' flavour (no density_grid) and a bare state_dict
    full = checkpoint.save_model(src, str(tmp_path / "ngp_ep0007.pth"), epoch=7, global_step=700)
    best = checkpoint.save_model(src, str(tmp_path / "ngp.pth"), best=True)
    bare = str(tmp_path / "bare.pth")
    torch.save(src.state_dict(), bare)
    raw = torch.load(full, weights_only=False)
    assert set(raw) >= {"epoch", "global_step", "stats", "model", "mean_count", "mean_density"} and set(raw["model"]) == set(_layout()["nerf"])

    dst = network.NeRFNetwork(bound=2, cuda_ray=True)
    info = checkpoint.load_model(dst, full)
    assert info["missing"] == [] and info["unexpected"] == [] and info["epoch"] == 7 and dst.mean_count == 4321 and dst.mean_density == 0.125
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    dst2 = network.NeRFNetwork(bound=2, cuda_ray=True)
    info = checkpoint.load_model(dst2, best)
    assert info["missing"] == ["density_grid"] and torch.equal(dst2.density_bitfield, src.density_bitfield)
    dst3 = network.NeRFNetwork(bound=2, cuda_ray=True)
    assert checkpoint.load_model(dst3, bare)["bare"] and torch.equal(dst3.encoder.embeddings, src.encoder.embeddings)
    # PaletteNeRF starts from a trained NeRF checkpoint: the shared sub-modules load, the palette heads are reported missing
    pal = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True)
    info = checkpoint.load_model(pal, full)
    assert info["unexpected"] == [] and "basis_color" in info["missing"] and torch.equal(pal.sigma_net[1].weight, src.sigma_net[1].weight)
    assert torch.equal(pal.encoder.embeddings, src.encoder.embeddings)
    with pytest.raises(RuntimeError):  # a bare state_dict loads strictly, like the reference
        checkpoint.load_model(network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True), bare)


# ------------------------------------------------------------------ f2: get_rays
def test_get_rays_oracle_and_index_selection_against_the_reference():
    """tests/golden/get_rays.npz holds outputs of the reference's own get_rays (nerf/utils.py:53-149, run on CPU by gen_golden.py):
    the oracle's ray arithmetic within 1e-6 of torch's, and the mirror's pixel selection identical under the same torch seed."""
    from palettenerf_amd import rays
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "get_rays.npz"))
    H, W = [int(v) for v in g["HW"]]
    o, d = oracle.get_rays(g["poses"], g["intrinsics"], H, W)
    np.testing.assert_allclose(d, g["full_d"], atol=1e-6, rtol=0)
    np.testing.assert_array_equal(o, g["full_o"])
    o, d = oracle.get_rays(g["poses"], g["intrinsics"], H, W, g["rand_inds"])
    np.testing.assert_allclose(d, g["rand_d"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(oracle.get_rays(g["poses"], g["intrinsics"], H, W, g["err_inds"])[1], g["err_d"], atol=1e-6, rtol=0)
    torch.manual_seed(12)
    np.testing.assert_array_equal(rays._patch_indices(H, W, 64, 4, "cpu").numpy(), g["patch_inds"][0])
    torch.manual_seed(13)
    np.testing.assert_array_equal(rays._pair_indices(H, W, 64, 3, "cpu").numpy(), g["pair_inds"][0])


def uniform_sampling_frames(case, out):
    """The frame of run_nerf_<case>.npz through the mirror's run() and its staged render() dispatcher, written to `out` (.npz); needs the facade."""
    g = np.load(os.path.join(GOLDEN, f"run_nerf_{case}.npz"))
    m = network.NeRFNetwork(bound=2, cuda_ray=False, density_scale=float(g["density_scale"]), min_near=0.2)
    scene.seed_field_(m, int(g["seed"]))
    m.eval()
    ro, rd = rays(g)
    kw = dict(num_steps=int(g["num_steps"]), upsample_steps=int(g["upsample_steps"]), perturb=False)
    with torch.no_grad():
        r = m.run(ro, rd, **kw)
        rs = m.render(ro, rd, staged=True, max_ray_batch=100, **kw)
    np.savez(out, **{k: r[k].numpy() for k in ("image", "depth", "weights_sum")}, **{"staged_" + k: rs[k].numpy() for k in ("image", "depth", "weights_sum")})


@pytest.mark.parametrize("case", ["a", "b"])
def test_uniform_sampling_path_reproduces_the_reference_run(case, tmp_path):
    """BASELINE configs[0]: NeRFRenderer.run without an occupancy grid (nerf/renderer.py:127-255) -- goldens made by the reference's own
    run() (tests/golden/gen_golden.py run).  Both the direct call and the staged render() dispatcher (4096-ray batches in the reference,
    small ones here) must give the frame.  The frame is rendered in a child process under gen_golden.PINNED_CPU_ENV, the CPU arithmetic the
    goldens were recorded under: the upsampling's inverse CDF turns the last-bit differences of a host's vector kernels into 5e-5 on a few pixels."""
    import importlib.util
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(GOLDEN, "gen_golden.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    out = str(tmp_path / "frames.npz")
    code = (f"import sys; sys.path.insert(0, {root!r}); from tests import test_host_logic as t; t.install_facade(); "
            f"t.uniform_sampling_frames({case!r}, {out!r})")
    p = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **gg.PINNED_CPU_ENV), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    g = np.load(os.path.join(GOLDEN, f"run_nerf_{case}.npz"))
    r = {k: torch.from_numpy(got[k]) for k in ("image", "depth", "weights_sum")}
    rs = {k: torch.from_numpy(got["staged_" + k]) for k in ("image", "depth", "weights_sum")}
    for k in ("image", "depth", "weights_sum"):
        np.testing.assert_allclose(r[k].numpy(), g[k], rtol=0, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(rs[k].numpy(), g[k], rtol=0, atol=2e-6, err_msg="staged " + k)


def test_sample_pdf_matches_a_direct_inverse_cdf():
    """sample_pdf (nerf/renderer.py:12-45): deterministic mode against a NumPy float64 inverse CDF of the same piecewise-constant density."""
    rng = np.random.default_rng(5)
    bins = np.sort(rng.uniform(0.2, 4.0, size=(7, 33)), axis=1).astype(np.float32)
    w = rng.uniform(0, 1, size=(7, 32)).astype(np.float32)
    w[2] = 0.0          # an empty ray: uniform over its bins
    w[3, 5:] = 0.0
    got = renderer.sample_pdf(torch.from_numpy(bins), torch.from_numpy(w), 16, det=True).numpy()
    pdf = (w.astype(np.float64) + 1e-5)
    pdf /= pdf.sum(1, keepdims=True)
    cdf = np.concatenate([np.zeros((7, 1)), np.cumsum(pdf, 1)], 1)
    u = np.linspace(0.5 / 16, 1 - 0.5 / 16, 16)
    for b in range(7):
        want = np.interp(u, cdf[b], bins[b].astype(np.float64))   # cdf has 33 knots: bins are the abscissae
        flat = np.diff(cdf[b]) < 1e-5                               # the reference treats a (nearly) empty bin as width 1 in cdf space
        ok = ~flat[np.clip(np.searchsorted(cdf[b], u, side="right") - 1, 0, 31)]
        np.testing.assert_allclose(got[b][ok], want[ok], rtol=0, atol=2e-4)
    assert np.all(np.diff(got, axis=1) >= -1e-6)


def test_palette_weight_lut_is_a_trilinear_lookup():
    """get_palette_weight_with_hist (palette/utils.py:117-124) against a direct NumPy trilinear interpolation of the [R, G, B] LUT, and against the
    reference's own expression (grid_sample over rgb[..., [2, 1, 0]] * 2 - 1)."""
    from palettenerf_amd import palette_utils
    rng = np.random.default_rng(3)
    nb, R = 4, 8
    lut = rng.random((nb, R, R, R)).astype(np.float32)
    rgb = rng.random((5, 7, 3)).astype(np.float32)
    rgb[0, 0] = [0.0, 1.0, 0.5]
    hw = torch.from_numpy(lut)[None]
    got = palette_utils.get_palette_weight_with_hist(torch.from_numpy(rgb), hw).numpy()
    assert got.shape == (5, 7, nb)
    p = rgb.reshape(-1, 3).astype(np.float64) * (R - 1)
    i0 = np.clip(np.floor(p).astype(int), 0, R - 2)
    f = p - i0
    want = np.zeros((p.shape[0], nb))
    for dr in (0, 1):
        for dg in (0, 1):
            for db in (0, 1):
                wgt = np.where(dr, f[:, 0], 1 - f[:, 0]) * np.where(dg, f[:, 1], 1 - f[:, 1]) * np.where(db, f[:, 2], 1 - f[:, 2])
                want += wgt[:, None] * lut[:, i0[:, 0] + dr, i0[:, 1] + dg, i0[:, 2] + db].T
    np.testing.assert_allclose(got.reshape(-1, nb), want, rtol=0, atol=2e-6)
    t = torch.from_numpy(rgb).reshape(-1, 3)
    ref = torch.nn.functional.grid_sample(hw, t[None, None, None, :, [2, 1, 0]] * 2 - 1, mode="bilinear", padding_mode="zeros", align_corners=True)
    np.testing.assert_array_equal(got.reshape(-1, nb), ref.squeeze().permute(1, 0).numpy())


def test_stylizer_matches_its_formula_and_starts_as_the_plain_composite():
    """Stylizer (palette/renderer.py:150-183): with its initial parameters it is the plain colour-basis composite with clamping
    sum_b omega_b clamp(softplus(radiance) (P_b + offsets_b), 0, 1) + view_dep; with perturbed parameters it follows the reference's expression."""
    import torch.nn.functional as F
    opt = renderer.default_opt()
    st = renderer.Stylizer(opt)
    assert {k: tuple(v.shape) for k, v in st.state_dict().items()} == {"dI": (4,), "dP": (1, 4, 3), "ddelta": (4, 3, 3)}
    g = torch.Generator().manual_seed(4)
    M, nb = 50, opt.num_basis
    radiance, omega = torch.randn(M, 1, 1, generator=g), torch.rand(M, nb, 1, generator=g)
    palette, offsets, vd = torch.rand(1, nb, 3, generator=g), torch.randn(M, nb, 3, generator=g) * 0.1, torch.rand(M, 3, generator=g)
    plain = (omega * (F.softplus(radiance) * (palette + offsets)).clamp(0, 1)).sum(-2) + vd
    torch.testing.assert_close(st(radiance, omega, palette.expand(M, nb, 3), offsets, vd), plain)
    assert float(st.ARAP_loss()) == 0.0
    with torch.no_grad():
        st.dI.copy_(torch.tensor([0.1, -0.2, 0.0, 0.3])); st.dP.normal_(0, 0.05, generator=g); st.ddelta.add_(torch.randn(nb, 3, 3, generator=g) * 0.1)
    want = ((F.softplus(radiance).repeat(1, nb, 1) + st.dI[None, :, None]).clamp(0)
            * ((palette.expand(M, nb, 3) + st.dP) + torch.einsum("npi,pij->npj", offsets, st.ddelta))).clamp(0, 1)
    want = (omega * want).sum(-2)
    torch.testing.assert_close(st(radiance, omega, palette.expand(M, nb, 3), offsets), want)
    assert float(st.ARAP_loss()) > 0.0


# ------------------------------------------------------------------ several frames in flight (host side of palettenerf_amd/pipeline.py)
def test_concurrent_frame_handles_share_weights_and_refuse_the_cpu():
    """clone_for_concurrent_frames: the extra handle shares every Parameter and buffer object with the model (no copy) and owns a fused-field
    object of its own with the model's settings; FramesInFlight has no CPU path and says so."""
    from palettenerf_amd.fused import NeRFFieldFused
    from palettenerf_amd.pipeline import FramesInFlight, clone_for_concurrent_frames
    m = network.NeRFNetwork(bound=2, cuda_ray=True)
    with pytest.raises(RuntimeError):
        clone_for_concurrent_frames(m)                      # no fused field yet
    m._fused = NeRFFieldFused(m)
    m._fused.precision = 0
    m._fused.ray_order = torch.arange(4, dtype=torch.int32)
    twin = clone_for_concurrent_frames(m)
    assert twin is not m and twin._fused is not m._fused and twin._fused.model is twin
    assert twin._fused.precision == 0 and twin._fused.ray_order is m._fused.ray_order
    for (na, pa), (nb_, pb) in zip(m.named_parameters(), twin.named_parameters()):
        assert na == nb_ and pa is pb
    assert twin.density_bitfield is m.density_bitfield
    assert m._fused.model is m                              # the original is untouched
    with pytest.raises(RuntimeError):
        FramesInFlight(m, 2)                                # CPU model: the product path is the HIP library, nothing else


def test_cached_zero_maps_are_replaced_once_written_and_parameter_keys_memoise_inside_a_held_call():
    """Host-side caches of the native frame path (no GPU needed): renderer._zero_map hands out one all-zero tensor per shape until somebody writes into it
    (torch's version counter), fused._pkey forms a tensor's key once inside a held call and afresh outside, fused._weight_of returns what attribute access
    returns."""
    from palettenerf_amd import fused
    from palettenerf_amd.renderer import _zero_map

    class Owner:
        pass
    o, like = Owner(), torch.zeros(1)
    a = _zero_map(o, "clip_feat", (5, 3), like)
    assert a.shape == (5, 3) and float(a.abs().sum()) == 0.0
    assert _zero_map(o, "clip_feat", (5, 3), like) is a                     # cached
    assert _zero_map(o, "clip_feat", (6, 3), like) is not a                 # another shape
    b = _zero_map(o, "clip_feat", (6, 3), like)
    b.add_(1.0)                                                             # a caller scribbles on the map ...
    c = _zero_map(o, "clip_feat", (6, 3), like)
    assert c is not b and float(c.abs().sum()) == 0.0                       # ... the next frame gets a clean one
    assert _zero_map(o, "rgb_norm", (6, 3), like) is not c                  # names do not share entries

    m = network.NeRFNetwork(bound=1, cuda_ray=False)
    assert fused._weight_of(m, "sigma_net", 1) is m.sigma_net[1].weight and fused._weight_of(m, "color_net", 2) is m.color_net[2].weight
    w = m.sigma_net[0].weight
    k0 = fused._pkey(w)
    f = fused.NeRFFieldFused(m)
    with f._held():
        k1 = fused._pkey(w)
        with torch.no_grad():
            w.add_(1.0)                                                     # (inside a held call the key is not re-read: the call's own answers stay consistent)
        assert fused._pkey(w) is k1 and k1 == k0
    assert fused._pkey(w) != k0                                             # outside: the version counter moved
