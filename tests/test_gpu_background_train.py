"""Training the background model (bg_radius > 0) on the fused path: pnr_background_train_forward / pnr_background_backward behind
BackgroundFused.train_from_rays / train_from_coords, the routing switch `fused_train_background`, and train_loss with a per-ray background that
needs a gradient (pnr_train_loss_backward_bg).

Reference.  Float64 throughout, at the DEVICE's own sphere coordinates (raymarching.sph_from_ray, which the kernel reproduces bit for bit):
tests/grid_reference.py for the 2-D table (lookup and table gradient), plain float64 torch for SH, the two layers, ReLU and sigmoid.  The code
under test is never its own reference.

The bound on a gradient is BOUND = 4 x E of the largest entry of the reference gradient, and never looser than GRAD_TOL = 4e-5, the project's figure
for these operators (tests/test_gpu_background.py): min(GRAD_TOL, 4 x E).  E is the error of the per-op formulation (`fused_train_background = False`:
GridEncoder, SHEncoder, the dense layers and autograd's backward of them) against the same float64 evaluation on the same inputs.  Every test below
prints both errors, and the per-op error is held to the recorded E.
Measured on the MI355X over the shapes of CASES (profiles/background_train/README.md), the same in every run:
    E = 8.62e-7 (bg_net.0.weight, 512 copies of one ray; table gradient at most 3.89e-7, bg_net.1.weight 1.96e-7), so BOUND = 3.45e-6.
    The fused path's own worst figures: 4.51e-7 against float64; 2.5e-6 for a whole 32 x 32 NeRF step against the per-op branch (sigma_net.1.weight).
Colours: KERNEL_TOL = 1e-5 as in tests/test_gpu_background.py."""
import functools

import numpy as np
import pytest
import torch

from oracle.torch_encoders import TorchSHEncoder
from palettenerf_amd import _lib, dropin, optim, raymarching
from palettenerf_amd.fused import background_fused
from palettenerf_amd.train_loss import TrainResults, train_loss
from tests import grid_reference as gr
from tests.test_gpu_background import COLOUR_TOL, GRAD_TOL, KERNEL_TOL, KW, frame_rays, make_model, rays_outside_in
from tests.test_train_loss import LAM, make_raw, torch_loss

pytestmark = pytest.mark.gpu

E_PER_OP = 8.62e-7       # measured, see the module docstring
BOUND = min(GRAD_TOL, 4 * E_PER_OP)
PARAMS = ("encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight")
CASES = ("n1", "n63", "n257", "n1000", "n8192", "same512", "oob", "dead")
DEAD_ALWAYS = (5, 40)     # hidden units of the "dead" model that no ray can switch on


@functools.lru_cache(maxsize=None)
def model(dead=False):
    m = make_model("nerf", torch.device("cuda:0"), 21, 1.0, bg_scale=1.0).train()
    if dead:
        with torch.no_grad():
            w = m.bg_net[0].weight
            w[3::4].neg_()                            # every fourth unit sees the negated pre-activation: dead on the rays that had it alive
            for j in DEAD_ALWAYS:                     # SH's first feature is the constant 0.282: these units are dead on every ray
                w[j, 0] = -40.0
    return m


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (rays_o or None, rays_d, coords, grad_rgb): device tensors.  The coordinates are sph_from_ray's, except for "oob"."""
    cuda = torch.device("cuda:0")
    n = {"same512": 512, "oob": 256, "dead": 257}.get(case) or int(case[1:])
    o, d = rays_outside_in(cuda, n, seed=len(case) + n)
    if case == "same512":
        o, d = o[:1].expand(n, 3).contiguous(), d[:1].expand(n, 3).contiguous()
    coords = raymarching.sph_from_ray(o, d, 4)
    if case == "oob":        # a quarter of the rays carries coordinates outside [-1, 1] (one of them, the other, or both)
        coords = coords.clone()
        coords[0::12, 0] = 1.25
        coords[4::12, 1] = -1.5
        coords[8::12] = torch.tensor([-1.0000001, 3.0], device=cuda)
        o = None
    weight = torch.rand(n, 3, generator=torch.Generator().manual_seed(n)).to(cuda) - 0.3
    return o, d, coords, weight


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64: colours [N,3], the three parameter gradients of sum(rgb * grad_rgb) and the table rows some ray touches."""
    m = model(case == "dead")
    _, d, coords, weight = inputs(case)
    e = m.encoder_bg
    x01 = ((coords.cpu().numpy() + np.float32(1)) / np.float32(2)).astype(np.float32)
    G = gr.GridReference(x01, e.offsets.cpu().numpy(), float(e.per_level_scale), e.base_resolution, e.gridtype_id, bool(e.align_corners))
    feat, _ = G.forward(e.embeddings.detach().cpu().numpy())
    feat = torch.from_numpy(feat.reshape(len(x01), -1)).requires_grad_(True)
    w0 = m.bg_net[0].weight.detach().double().cpu().requires_grad_(True)
    w1 = m.bg_net[1].weight.detach().double().cpu().requires_grad_(True)
    h = torch.cat([TorchSHEncoder(degree=4)(d.double().cpu()), feat], dim=-1)
    rgb = torch.sigmoid(torch.relu(h @ w0.T) @ w1.T)
    (rgb * weight.double().cpu()).sum().backward()
    g_table, _, touched = G.table_grad(feat.grad.numpy())
    return {"rgb": rgb.detach().numpy(), PARAMS[0]: g_table, PARAMS[1]: w0.grad.numpy(), PARAMS[2]: w1.grad.numpy(), "touched": touched > 0,
            "in_range": G.inr}


def run(case, fused, autocast=False, weight=None):
    """One forward + backward through the model's own call sites -> (rgb, {parameter: gradient}) as float64 numpy."""
    m = model(case == "dead")
    o, d, coords, w = inputs(case)
    w = w if weight is None else weight
    m.zero_grad(set_to_none=True)
    m.fused_train_background = fused
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            rgb = m._background_of_rays(o, d) if o is not None else m.background(coords, d)
            (rgb.float() * w).sum().backward()
    finally:
        m.fused_train_background = True
    named = dict(m.named_parameters())
    return rgb.detach().double().cpu().numpy(), {k: named[k].grad.detach().double().cpu().numpy() for k in PARAMS}


def rel_err(got, want):
    scale = float(np.abs(want).max())
    assert scale > 0
    return float(np.abs(got - want).max()) / scale


def calls_of(fn):
    names = []
    real = _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        out = fn()
    finally:
        _lib.call = real
    return names, out


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("case", ["n1", "n63", "n257", "n1000", "oob"])
def test_forward_is_the_inference_launch_bit_for_bit(cuda, case):
    m = model()
    o, d, coords, _ = inputs(case)
    bgf = background_fused(m)
    with torch.no_grad():
        want = bgf.from_coords(coords, d, half=False)
    got = bgf.train_from_coords(coords, d)
    assert got.requires_grad and got.dtype == torch.float32 and torch.equal(got, want)
    if o is not None:
        with torch.no_grad():
            want_rays = bgf.from_rays(o, d, half=False)
        got_rays, saved = bgf.train_from_rays(o, d, want_coords=True)
        assert torch.equal(got_rays, want_rays) and torch.equal(got_rays, got)
        assert torch.equal(saved, raymarching.sph_from_ray(o, d, m.bg_radius)) and not saved.requires_grad


# ---------------------------------------------------------------- gradients against float64
@pytest.mark.parametrize("case", CASES)
def test_gradients_against_float64(cuda, case):
    ref = reference(case)
    names, (rgb, grads) = calls_of(lambda: run(case, True))
    assert names.count("pnr_background_train_forward") == 1 and names.count("pnr_background_backward") == 1
    assert not any(n.startswith(("pnr_grid_encode", "pnr_sh_encode", "pnr_background_pack")) for n in names)
    _, per_op = run(case, False)
    assert float(np.abs(rgb - ref["rgb"]).max()) <= KERNEL_TOL
    for k in PARAMS:
        e_fused, e_per_op = rel_err(grads[k], ref[k]), rel_err(per_op[k], ref[k])
        print(f"{case} {k}: fused {e_fused:.3g}, per-op {e_per_op:.3g} of max |g| {np.abs(ref[k]).max():.3g}")
        assert e_per_op <= E_PER_OP, (k, "the per-op formulation is further from float64 than the recorded E")
        assert e_fused <= BOUND, k
    table = grads[PARAMS[0]]
    assert ref["touched"].any() and not table[~ref["touched"]].any()          # rows no ray touches: exactly zero
    if case == "oob":
        out = ~ref["in_range"]
        assert out.sum() == 64                                                    # a quarter of the 256
        # the out-of-range rays alone: nothing in the table, nothing in the table columns of bg_net.0.weight
        o, d, coords, w = inputs(case)
        m = model()
        m.zero_grad(set_to_none=True)
        idx = torch.from_numpy(np.nonzero(out)[0]).to(cuda)
        (m.background(coords[idx].contiguous(), d[idx].contiguous()) * w[idx]).sum().backward()
        assert not m.encoder_bg.embeddings.grad.any() and not m.bg_net[0].weight.grad[:, 16:].any()
        assert float(m.bg_net[0].weight.grad[:, :16].abs().sum()) > 0
    if case == "dead":
        dead = list(DEAD_ALWAYS)
        assert not ref[PARAMS[1]][dead].any() and not grads[PARAMS[1]][dead].any() and not grads[PARAMS[2]][:, dead].any()
        assert np.abs(ref[PARAMS[1]][3::4]).max() > 0


def test_zero_grad_rgb_gives_exactly_zero(cuda):
    _, grads = run("n257", True, weight=torch.zeros(257, 3, device=cuda))
    for k in PARAMS:
        assert not grads[k].any(), k


@pytest.mark.parametrize("case", ["n1000", "n8192", "same512"])
def test_weight_gradients_are_bitwise_reproducible(cuda, case):
    _, a = run(case, True)
    _, b = run(case, True)
    for k in PARAMS[1:]:
        assert np.array_equal(a[k], b[k]), k
    if case == "same512":     # every wave sums the same 64 addends: the slabs are equal, and 512 x one ray's table rows
        assert np.count_nonzero(a[PARAMS[0]].any(axis=1)) <= 16


def test_double_backward_raises(cuda):
    m = model()
    _, d, coords, w = inputs("n63")
    rgb = m.background(coords, d)
    (g,) = torch.autograd.grad((rgb * rgb * w).sum(), m.bg_net[1].weight, create_graph=True)      # the incoming gradient itself needs one
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g.sum().backward()


def test_autocast_is_no_further_from_float64_than_the_per_op_path(cuda):
    ref = reference("n1000")
    rgb_f, g_f = run("n1000", True, autocast=True)
    rgb_p, g_p = run("n1000", False, autocast=True)
    e_f, e_p = float(np.abs(rgb_f - ref["rgb"]).max()), float(np.abs(rgb_p - ref["rgb"]).max())
    print(f"autocast colours: fused {e_f:.3g}, per-op {e_p:.3g}")
    assert e_f <= e_p and e_f <= KERNEL_TOL
    for k in PARAMS:
        e_f, e_p = rel_err(g_f[k], ref[k]), rel_err(g_p[k], ref[k])
        print(f"autocast {k}: fused {e_f:.3g}, per-op {e_p:.3g}")
        assert e_f <= e_p, k


# ---------------------------------------------------------------- train_loss with a background that needs a gradient
@pytest.mark.parametrize("palette, clip", [(False, 0), (True, 0), (True, 8)])
def test_train_loss_sends_the_background_its_gradient(cuda, palette, clip):
    N = 257
    raw, gt, gt_clip, gt_w = make_raw(N, 4, clip, "map", cuda, seed=3, palette=palette)
    kw = dict(lambda_sparsity=LAM["sparsity"], lambda_offsets=LAM["offsets"], lambda_view_dep=LAM["view_dep"], lambda_smooth=LAM["smooth"],
              lambda_weight=LAM["weight"], gt_weights=gt_w, gt_clip=gt_clip) if palette else {}
    leaves = [t for t in (raw.weights_sum, raw.image_raw, raw.all_map) if t is not None]
    loss0, info0 = train_loss(TrainResults(raw), gt, **kw)
    g0 = torch.autograd.grad(loss0 * 1.5, leaves)
    bg = raw.bg_color.clone().requires_grad_(True)
    names, (loss1, info1) = calls_of(lambda: train_loss(TrainResults(raw._replace(bg_color=bg)), gt, **kw))
    assert names == ["pnr_train_loss_forward"]
    names, g1 = calls_of(lambda: torch.autograd.grad(loss1 * 1.5, leaves + [bg]))
    assert names == ["pnr_train_loss_backward", "pnr_train_loss_backward_bg"]
    assert torch.equal(loss0, loss1)
    for k in ("terms", "loss_ray", "image", "depth", "direct_rgb"):
        assert (info0[k] is None and info1[k] is None) or torch.equal(info0[k], info1[k]), k
    assert (info1["direct_rgb"] is not None) == palette
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # float64, the torch formulation of the loss on the dict entries
    f64 = lambda t: None if t is None or not torch.is_tensor(t) else t.detach().double().cpu()   # noqa: E731
    bg64 = f64(bg).requires_grad_(True)
    raw64 = raw._replace(**{k: f64(getattr(raw, k)) for k in ("weights_sum", "depth_raw", "image_raw", "all_map", "nears", "fars")}, bg_color=bg64)
    lam = dict(LAM, palette=0.0)
    loss64, _ = torch_loss(TrainResults(raw64), f64(gt), lam, f64(gt_clip), f64(gt_w))
    (want,) = torch.autograd.grad(loss64 * 1.5, bg64)
    err = rel_err(g1[-1].double().cpu().numpy(), want.numpy())
    print(f"grad_bg palette={palette} clip={clip}: rel err {err:.3g}")
    assert g1[-1].shape == bg.shape and err <= BOUND
    # a trainable [3] background is not this path
    raw3 = raw._replace(bg_color=torch.rand(3, device=cuda, requires_grad=True))
    with pytest.raises(RuntimeError, match="per ray"):
        train_loss(TrainResults(raw3), gt, **kw)


# ---------------------------------------------------------------- one whole training step
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_whole_training_step_matches_the_per_op_branch(cuda, kind):
    m = make_model(kind, cuda, 23, 1.0, bg_scale=1.0).train()
    ro, rd = frame_rays(cuda, 32, 32)
    gt = torch.rand(1, 32 * 32, 3, generator=torch.Generator().manual_seed(9)).to(cuda)
    bco = (m.basis_color.detach() + 0.05).clone() if kind == "palette" else None

    def step(fused):
        m.zero_grad(set_to_none=True)
        m.fused_train_background = fused
        r = m.run_cuda(ro, rd, dt_gamma=0.0, perturb=False, force_all_rays=True, **KW)
        assert r.raw.bg_color.requires_grad and tuple(r.raw.bg_color.shape) == (32 * 32, 3)
        if not fused:
            loss, _ = torch_loss(r, gt.reshape(-1, 3), dict(LAM, smooth=0.0, weight=0.0), bc=m.basis_color if bco is not None else None, bco=bco)
        elif kind == "palette":
            loss, _ = train_loss(r, gt, lambda_sparsity=LAM["sparsity"], lambda_offsets=LAM["offsets"], lambda_view_dep=LAM["view_dep"],
                                 lambda_palette=LAM["palette"], basis_color=m.basis_color, basis_color_origin=bco)
        else:
            loss, _ = train_loss(r, gt)
        loss.backward()
        return float(loss), {n: p.grad.detach().double().cpu().numpy() for n, p in m.named_parameters() if p.grad is not None}

    names, (l_fused, g_fused) = calls_of(lambda: step(True))
    assert {"pnr_background_train_forward", "pnr_background_backward", "pnr_train_loss_backward_bg"} <= set(names)
    l_ref, g_ref = step(False)
    m.fused_train_background = True
    assert abs(l_ref - l_fused) <= 2e-6 * abs(l_ref)
    assert set(g_ref) == set(g_fused) and set(PARAMS) <= set(g_fused)
    for name in g_ref:
        err = rel_err(g_fused[name], g_ref[name])
        print(f"{kind} {name}: rel err {err:.3g}")
        assert err <= BOUND, name


# ---------------------------------------------------------------- fallbacks, drop-in, optimiser
def test_switch_off_and_inputs_with_gradients_take_the_per_op_path(cuda):
    m = model()
    o, d, coords, w = inputs("n257")

    def go(x, dirs, rays=False):
        m.zero_grad(set_to_none=True)
        out = m._background_of_rays(x, dirs) if rays else m.background(x, dirs)
        (out * w).sum().backward()
        return out

    for rays in (False, True):
        names, _ = calls_of(lambda: go(o if rays else coords, d, rays))
        assert "pnr_background_train_forward" in names and "pnr_background_backward" in names
        m.fused_train_background = False
        try:
            names, _ = calls_of(lambda: go(o if rays else coords, d, rays))
        finally:
            m.fused_train_background = True
        assert not any(n.startswith("pnr_background") for n in names) and any(n.startswith("pnr_grid_encode_forward") for n in names)
    x = coords.clone().requires_grad_(True)
    names, _ = calls_of(lambda: go(x, d))
    assert not any(n.startswith("pnr_background") for n in names) and any(n.startswith("pnr_grid_encode_forward") for n in names)
    with torch.no_grad():                                  # inference keeps its own launch
        names, _ = calls_of(lambda: m.background(coords, d))
    assert names[-1] == "pnr_background_forward" and "pnr_background_train_forward" not in names


def test_fuse_field_trains_the_background_and_unfuse_unbinds(cuda):
    m = make_model("palette", cuda, 25, 1.0, bg_scale=1.0).train()
    m.march_mode, m.fused_field = "compat", False
    _, d, coords, w = inputs("n257")
    ref = None

    def go():
        m.zero_grad(set_to_none=True)
        (m.background(coords, d) * w).sum().backward()
        return {k: dict(m.named_parameters())[k].grad.clone() for k in PARAMS}

    names, ref = calls_of(go)
    assert not any(n.startswith("pnr_background") for n in names)
    dropin.fuse_field(m)
    names, got = calls_of(go)
    assert "background" in m.__dict__ and "pnr_background_train_forward" in names and "pnr_background_backward" in names
    for k in PARAMS:
        assert float((got[k] - ref[k]).abs().max()) <= BOUND * float(ref[k].abs().max()), k
    m.fused_train_background = False
    names, _ = calls_of(go)
    assert not any(n.startswith("pnr_background") for n in names)
    m.fused_train_background = True
    dropin.unfuse(m)
    names, _ = calls_of(go)
    assert "background" not in m.__dict__ and not any(n.startswith("pnr_background") for n in names)


def test_adam_step_then_inference_reads_the_live_weights(cuda):
    ro, rd = frame_rays(cuda, 32, 32)
    _, d, coords, w = inputs("n1000")
    frames = {}
    for fused in (True, False):
        m = make_model("nerf", cuda, 27, 1.0, bg_scale=1.0)
        m.fused_train_background = fused
        with torch.no_grad():
            before = m.render(ro, rd, dt_gamma=0.0, perturb=False, **KW)["image"].clone()      # (packs the inference blob before the step)
        opt = optim.Adam(m.get_params(1e-2)[-2:], betas=(0.9, 0.99), eps=1e-15)       # the two background groups
        for _ in range(2):
            opt.zero_grad()
            (m.background(coords, d) * w).sum().backward()
            opt.step()
        with torch.no_grad():
            frames[fused] = m.render(ro, rd, dt_gamma=0.0, perturb=False, **KW)["image"]
        assert float((frames[fused] - before).abs().max()) > 10 * COLOUR_TOL
    err = float((frames[True] - frames[False]).abs().max())
    print(f"frame after two Adam steps, fused against per-op twin: {err:.3g}")
    assert err <= COLOUR_TOL
