"""The smooth-loss block of a PaletteNeRF training step on its HIP kernels (pnr_palette_smooth_*; palette/renderer.py:360-378): the three entries
against the reference block evaluated in float64, smooth_branch against forward(), and the training step with fused_train_smooth on and off."""
import functools
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 257)        # one lane, one wave minus / exactly / plus one, more than one 256-row workgroup
SIGMA_XYZ, SIGMA_COLOR = 0.005, 0.2      # main_palette.py's defaults
# (clip_dim, sigma_clip): no clip head; a head outside the weight; the quirk (norm, not squared) in the weight; a row wider than the 32-column
# LDS chunk with an odd tail; the widest row the entry takes
CLIPS = {"none": (0, 0.0), "clip16_sigma0": (16, 0.0), "clip16_sigma0.5": (16, 0.5), "clip40_sigma0.5": (40, 0.5), "clip128_sigma0.5": (128, 0.5)}
CASES = [(nb, c) for nb in (1, 4, 16) for c in ("none", "clip16_sigma0", "clip16_sigma0.5")] + [(4, "clip40_sigma0.5"), (16, "clip128_sigma0.5")]


def reference_block(xyzs, xyzs_diff, diffuse, diffuse_diff, omega, omega_diff, clip_feat, clip_feat_diff, bound, sigma_clip):
    """palette/renderer.py:365-378 as written there (pred_clip = clip_feat is not None), in the dtype of its inputs.  -> smooth_norm, smooth_weight"""
    M, nb = omega.shape
    omega, omega_diff = omega.reshape(M, nb, 1), omega_diff.reshape(M, nb, 1)
    xyzs_weight = (xyzs - xyzs_diff).norm(dim=-1, keepdim=True) ** 2 / bound ** 2 / SIGMA_XYZ
    rgb_weight = (diffuse - diffuse_diff).norm(dim=-1, keepdim=True) ** 2 / SIGMA_COLOR
    if clip_feat is not None and sigma_clip > 0:
        clip_weight = (clip_feat - clip_feat_diff).norm(dim=-1, keepdim=True) / sigma_clip
    else:
        clip_weight = 0
    smooth_weight = torch.exp(-xyzs_weight - rgb_weight - clip_weight).detach()
    smooth_norm = ((omega_diff - omega)[..., 0] ** 2).sum(dim=-1, keepdim=True) * smooth_weight
    if clip_feat is not None:
        smooth_norm = smooth_norm + ((clip_feat_diff - clip_feat) ** 2).sum(dim=-1, keepdim=True) * smooth_weight
    return smooth_norm, smooth_weight


NAMES = ("xyzs", "xyzs_diff", "diffuse", "diffuse_diff", "omega", "omega_diff", "clip_feat", "clip_feat_diff")
GRAD_NAMES = ("omega", "omega_diff", "clip_feat", "clip_feat_diff")


@functools.lru_cache(maxsize=None)
def case(M, nb, clip_name):
    """Seeded inputs of one case (every fifth row: the pair is equal, so the norm is 0 and the weight exp(-xw)), the reference block's values and
    gradients in float64, and the error the same block shows in fp32 torch against them -- computed once, read by the forward and the backward test."""
    clip_dim, sigma_clip = CLIPS[clip_name]
    bound = {1: 1, 4: 2, 16: 24}[nb]
    g = torch.Generator().manual_seed(1000 * M + 10 * nb + clip_dim)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    xyzs = (r(M, 3) * 2 - 1) * bound
    xyzs_diff = (xyzs + r(M, 3) * bound * 0.03).clamp(-bound, bound)
    diffuse = r(M, 3)
    diffuse_diff = (diffuse + 0.1 * (r(M, 3) - 0.5)).clamp(0, 1)
    omega = r(M, nb) + 0.05
    omega = omega / omega.sum(-1, keepdim=True)
    omega_diff = r(M, nb) * 0.2 + omega
    omega_diff = omega_diff / omega_diff.sum(-1, keepdim=True)
    clip_feat = clip_feat_diff = None
    if clip_dim:
        clip_feat = r(M, clip_dim) - 0.5
        clip_feat_diff = clip_feat + 0.05 * (r(M, clip_dim) - 0.5)
    same = torch.arange(M) % 5 == 4
    diffuse_diff[same], omega_diff[same] = diffuse[same], omega[same]
    if clip_dim:
        clip_feat_diff[same] = clip_feat[same]
    g_norm = r(M, 1) + 0.1
    inputs = dict(zip(NAMES, (xyzs, xyzs_diff, diffuse, diffuse_diff, omega, omega_diff, clip_feat, clip_feat_diff)))

    def run(dtype):
        t = {k: None if v is None else v.cuda().to(dtype).requires_grad_(k in GRAD_NAMES) for k, v in inputs.items()}
        norm, weight = reference_block(*[t[k] for k in NAMES], bound, sigma_clip)
        norm.backward(g_norm.cuda().to(dtype))
        return dict(smooth_norm=norm.detach(), smooth_weight=weight.detach(), **{"grad_" + k: t[k].grad for k in GRAD_NAMES if t[k] is not None})

    ref64, ref32 = run(torch.float64), run(torch.float32)
    err32 = {k: float((ref32[k].double() - ref64[k]).abs().max()) for k in ref64}
    return dict(inputs=inputs, g_norm=g_norm, bound=bound, sigma_clip=sigma_clip, same=same, ref=ref64, ref32=ref32, err32=err32)


def rows_of(c, lo, hi):
    """The case restricted to rows [lo, hi): its inputs, its float64 values and the fp32 torch block's largest error on those rows alone."""
    cut = lambda v: None if v is None else v[lo:hi]      # noqa: E731
    ref = {k: cut(v) for k, v in c["ref"].items()}
    err32 = {k: float((cut(c["ref32"][k]).double() - ref[k]).abs().max()) for k in ref}
    return dict(c, inputs={k: cut(v) for k, v in c["inputs"].items()}, g_norm=cut(c["g_norm"]), same=cut(c["same"]), ref=ref, ref32=None, err32=err32)


def ulp32(v):
    return np.spacing(v.abs().float().cpu().numpy()).astype(np.float64)


def check(name, got, c, what):
    """|got - float64| <= 4 x (the fp32 torch block's largest error in this case) + one fp32 ulp of the column's largest value, per element."""
    ref = c["ref"][name]
    tol = 4 * c["err32"][name] + torch.from_numpy(ulp32(ref.abs().amax(dim=0))).to(ref.device)
    err = (got.double() - ref).abs()
    print(f"{what} {name}: max err {float(err.max()):.3e}  fp32-torch err {c['err32'][name]:.3e}  smallest tol {float(tol.min()):.3e}")
    assert bool((err <= tol).all()), (what, name, float(err.max()), c["err32"][name])


def fused(c, grads=True):
    from palettenerf_amd.palette_utils import palette_smooth
    t = {k: None if v is None else v.cuda().requires_grad_(grads and k in GRAD_NAMES) for k, v in c["inputs"].items()}
    norm = palette_smooth(*[t[k] for k in NAMES], c["bound"], SIGMA_XYZ, SIGMA_COLOR, c["sigma_clip"])
    return t, norm


@pytest.mark.parametrize("bound", [1, 2, 24])
def test_points_have_the_bits_of_the_torch_expression(cuda, bound):
    from palettenerf_amd.palette_utils import smooth_points
    for M in MS:
        g = torch.Generator().manual_seed(M + bound)
        xyzs = ((torch.rand(M, 3, generator=g) * 2 - 1) * bound)
        xyzs[::3, 0] = bound * (1 - 0.03 * torch.rand(xyzs[::3].shape[0], generator=g))   # within 0.03 bound of +bound: the clamp acts on most of these
        xyzs[1::4, 1] = -bound
        xyzs[2::7, 2] = bound
        xyzs, noise = xyzs.cuda(), torch.rand(M, 3, generator=g).cuda()
        noise[::5] = noise[::5].round()      # draws of exactly 0 (rand's range includes it) and the supremum
        if M > 5:
            noise[5] = 0                     # ... one of them at a sample that sits on -bound
        want = (xyzs + noise * bound * 0.03).clamp(-bound, bound)
        assert M < 3 or bool((want == bound).any() and (want == -bound).any())
        assert torch.equal(smooth_points(xyzs, noise, bound), want), (M, bound)
        assert torch.equal(smooth_points(xyzs, noise, float(bound)), want)
        # arrays that do not start on a 16-byte boundary take the element-wise path: same bits
        pad_x, pad_n = torch.zeros(M + 1, 3, device=cuda), torch.zeros(M + 1, 3, device=cuda)
        pad_x[1:], pad_n[1:] = xyzs, noise
        assert pad_x[1:].data_ptr() % 16 != 0
        assert torch.equal(smooth_points(pad_x[1:], pad_n[1:], bound), want), (M, bound, "unaligned")
    assert smooth_points(torch.zeros(0, 3, device=cuda), torch.zeros(0, 3, device=cuda), bound).shape == (0, 3)


@pytest.mark.parametrize("nb,clip_name", CASES)
def test_forward_against_the_float64_block(cuda, nb, clip_name):
    for M in MS:
        c = case(M, nb, clip_name)
        with torch.no_grad():
            _, norm = fused(c, grads=False)
        assert norm.shape == (M, 1) and norm.dtype == torch.float32
        check("smooth_norm", norm, c, (M, nb, clip_name))
        same = c["same"].cuda()
        assert bool((norm[same] == 0).all())                 # an equal pair: exactly no change
        # the weight the backward reads: through the entry itself
        from palettenerf_amd._torch_glue import call, ptr
        t = {k: None if v is None else v.cuda() for k, v in c["inputs"].items()}
        w, n2 = torch.empty(M, device=cuda), torch.empty(M, device=cuda)
        call("pnr_palette_smooth_forward", M, nb, CLIPS[clip_name][0], *[ptr(t[k]) for k in NAMES], float(c["bound"]), SIGMA_XYZ, SIGMA_COLOR,
             c["sigma_clip"], ptr(w), ptr(n2))
        check("smooth_weight", w.view(M, 1), c, (M, nb, clip_name))
        assert torch.equal(n2.view(M, 1), norm)


@pytest.mark.parametrize("nb,clip_name", CASES)
def test_backward_against_float64_autograd(cuda, nb, clip_name):
    for M in MS:
        c = case(M, nb, clip_name)
        t, norm = fused(c)
        norm.backward(c["g_norm"].cuda())
        for k in GRAD_NAMES:
            if t[k] is None:
                continue
            assert torch.isfinite(t[k].grad).all(), k      # also where clip_feat == clip_feat_diff: the quirk's norm has no finite derivative there
            check("grad_" + k, t[k].grad, c, (M, nb, clip_name))
        assert torch.equal(t["omega"].grad, -t["omega_diff"].grad)
        if t["clip_feat"] is not None:
            assert torch.equal(t["clip_feat"].grad, -t["clip_feat_diff"].grad)


def test_only_the_omega_and_clip_pairs_receive_a_gradient(cuda):
    from palettenerf_amd.palette_utils import palette_smooth
    c = case(65, 4, "clip16_sigma0.5")
    t = {k: v.cuda().requires_grad_(True) for k, v in c["inputs"].items()}
    norm = palette_smooth(*[t[k] for k in NAMES], c["bound"], SIGMA_XYZ, SIGMA_COLOR, c["sigma_clip"])
    norm.backward(c["g_norm"].cuda())
    for k in ("xyzs", "xyzs_diff", "diffuse", "diffuse_diff"):
        assert t[k].grad is None, k
    for k in GRAD_NAMES:
        assert t[k].grad is not None, k

    first = t["omega"].grad.clone()
    # a clip gradient nobody wants is not computed
    t = {k: v.cuda().requires_grad_(k in ("omega", "omega_diff")) for k, v in c["inputs"].items()}
    palette_smooth(*[t[k] for k in NAMES], c["bound"], SIGMA_XYZ, SIGMA_COLOR, c["sigma_clip"]).backward(c["g_norm"].cuda())
    assert t["clip_feat"].grad is None and torch.equal(t["omega"].grad, first)


# ------------------------------------------------------------------------------------------------ the network and the training step
def make_model(cuda, pred_clip):
    from palettenerf_amd import network, raymarching, renderer, scene
    m = network.PaletteNetwork(renderer.default_opt(test=False, pred_clip=pred_clip, smooth_sigma_clip=0.5 if pred_clip else 0.0), bound=2, cuda_ray=True,
                               min_near=0.02)
    scene.seed_field_(m, 0)
    m = m.to(cuda).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m


@functools.lru_cache(maxsize=None)
def rays64():
    from palettenerf_amd import scene
    H, W = 756, 1008
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]
    ro, rd = scene.get_rays(torch.from_numpy(pose)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    g = torch.Generator().manual_seed(5)
    inds = torch.randint(0, H * W, [64], generator=g)
    return ro[:, inds].cuda(), rd[:, inds].cuda(), torch.rand(1, 64, 3, generator=g).cuda()


@pytest.mark.parametrize("pred_clip", [False, True])
def test_smooth_branch_has_the_bits_of_forward(cuda, pred_clip):
    m = make_model(cuda, pred_clip)
    g = torch.Generator().manual_seed(11)
    x = ((torch.rand(1000, 3, generator=g) * 2 - 1) * 2).cuda()
    d = torch.nn.functional.normalize(torch.randn(1000, 3, generator=g), dim=-1).cuda()
    for frozen in (True, False):
        _, clip_feat, omega, _, _, diffuse = m(x, d, frozen_density=frozen)
        b_clip, b_omega, b_diffuse = m.smooth_branch(x, frozen_density=frozen)
        assert torch.equal(b_omega, omega) and torch.equal(b_diffuse, diffuse) and torch.equal(b_clip, clip_feat) and b_clip.shape == clip_feat.shape
        assert b_omega.requires_grad and (b_clip.requires_grad == bool(pred_clip))


LAM = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_smooth=4e-3)
# The project's rule for a gradient tolerance: 4 x the largest difference measured between the two formulations, as max |g_fused - g_torch| /
# max |g_torch| over the step's parameters.  Measured on an MI355X on this 64-ray step, four runs, per parameter in profiles/smooth/README.md
# ("Gradient agreement"): the MLP, head and palette gradients are bit-identical; the largest difference of each mode sits in a hash table's
# gradient (float atomics in arrival order at this batch size, half atomics under autocast) and is the constant below.
MEASURED_GRAD_DIFF = {"fp32": 1.823e-7, "fp32_clip": 4.703e-7, "fp16": 1.491e-3}


def train_step(m, fused_smooth, smooth=True, autocast=False, seed=7):
    from palettenerf_amd.train_loss import train_loss
    ro, rd, gt = rays64()
    m.require_smooth_loss, m.fused_train_smooth = smooth, fused_smooth
    seen = []
    fwd, branch = type(m).forward, type(m).smooth_branch
    m.forward = lambda x, d, **kw: (seen.append(x.detach().clone()), fwd(m, x, d, **kw))[1]
    m.smooth_branch = lambda x, **kw: (seen.append(x.detach().clone()), branch(m, x, **kw))[1]
    try:
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            r = m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=False, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
            loss, info = train_loss(r, gt, **LAM)
        (loss * (1024.0 if autocast else 1.0)).backward()
    finally:
        del m.forward, m.smooth_branch
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(points=seen, smooth_norm=r["smooth_norm"].detach().clone(), loss=loss.detach().clone(), loss_smooth=info["terms"][5].clone(), grads=grads,
                image=info["image"].clone())


@pytest.mark.parametrize("mode", ["fp32", "fp32_clip", "fp16"])
def test_training_step_fused_against_torch_smooth_block(cuda, mode):
    m = make_model(cuda, mode == "fp32_clip")
    a = train_step(m, True, autocast=mode == "fp16")
    b = train_step(m, False, autocast=mode == "fp16")
    assert len(a["points"]) == 2 and len(b["points"]) == 2
    assert torch.equal(a["points"][0], b["points"][0]) and torch.equal(a["points"][1], b["points"][1])      # xyzs and xyzs_diff: one seed, one perturbation
    assert not torch.equal(a["points"][0], a["points"][1]) and float(b["smooth_norm"].abs().max()) > 0
    scale = float(b["smooth_norm"].abs().max())
    d_map = float((a["smooth_norm"] - b["smooth_norm"]).abs().max())
    d_loss = abs(float(a["loss_smooth"]) - float(b["loss_smooth"]))
    print(f"{mode}: smooth_norm max diff {d_map:.3e} of max {scale:.3e}; loss_smooth {float(a['loss_smooth']):.6e} vs {float(b['loss_smooth']):.6e}")
    worst = 0.0
    assert set(a["grads"]) == set(b["grads"])
    for n in b["grads"]:
        ref = float(b["grads"][n].abs().max())
        rel = float((a["grads"][n] - b["grads"][n]).abs().max()) / ref if ref > 0 else 0.0
        print(f"{mode}: grad {n}: rel diff {rel:.3e} (max |g| {ref:.3e})")
        worst = max(worst, rel)
    print(f"{mode}: worst gradient rel diff {worst:.3e}")
    assert d_map <= 1e-4 * scale                                   # the contract: 1e-4 of the map's maximum
    assert d_loss <= 1e-4 * LAM["lambda_smooth"] * scale           # loss_smooth = lambda_smooth x the map's mean
    for n in b["grads"]:
        ref = float(b["grads"][n].abs().max())
        assert float((a["grads"][n] - b["grads"][n]).abs().max()) <= 4 * MEASURED_GRAD_DIFF[mode] * ref, n


@pytest.mark.parametrize("pred_clip", [False, True])
def test_without_the_smooth_loss_the_flag_changes_nothing(cuda, pred_clip, monkeypatch):
    """require_smooth_loss = False: the step's outputs and every gradient are the same bits whatever fused_train_smooth says.  A 64-ray batch is below
    gridencoder.BINNED_MIN_ROWS, where the table gradient is a scatter of float atomics in arrival order (two runs of ONE setting differ); the step
    takes the binned table gradient of a full-size batch instead, as tests/test_gpu_ops.py::test_grid_backward_binned_matches_oracle does."""
    from palettenerf_amd import gridencoder
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1)
    m = make_model(cuda, pred_clip)
    a, b = train_step(m, True, smooth=False), train_step(m, False, smooth=False)
    assert len(a["points"]) == 1 and torch.equal(a["loss"], b["loss"]) and torch.equal(a["image"], b["image"]) and torch.equal(a["smooth_norm"], b["smooth_norm"])
    assert float(a["smooth_norm"].abs().max()) == 0 and set(a["grads"]) == set(b["grads"]) and "encoder_palette.embeddings" in a["grads"]
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()            # warm: code objects, packed weights
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


@pytest.mark.parametrize("pred_clip", [False, True])
def test_fused_block_issues_fewer_launches_and_no_torch_elementwise_kernel(cuda, pred_clip):
    m = make_model(cuda, pred_clip)
    fused_names = kernel_names(lambda: train_step(m, True))
    torch_names = kernel_names(lambda: train_step(m, False))
    print(f"launches per 64-ray step: fused {len(fused_names)}, torch smooth block {len(torch_names)}")
    assert len(fused_names) < len(torch_names)
    first = [i for i, n in enumerate(fused_names) if "k_palette_smooth_points" in n]
    last = [i for i, n in enumerate(fused_names) if "k_palette_train_shade_fwd" in n]
    assert len(first) == 1 and len(last) == 1 and first[0] < last[0]
    between = fused_names[first[0] + 1:last[0]]
    assert sum("k_palette_smooth_fwd" in n for n in between) == 1
    # what smooth_branch launches by itself at those points (its lookups, MLP stacks and the x -> [0, 1] map in front of them) is not the block's
    x = train_step(m, True)["points"][1]
    own = Counter(kernel_names(lambda: m.smooth_branch(x)))
    rest = Counter(between) - own
    print("between smooth_points and palette_train_shade, beyond smooth_branch's own launches:", dict(rest))
    assert not [n for n in rest if "elementwise" in n.lower() or "at::native" in n or "reduce_kernel" in n], rest
    assert not any("k_palette_smooth" in n for n in torch_names)
