"""pnr_train_batch / pnr_error_map_update (csrc/train_batch.hip) and palettenerf_amd.trainset on the device, against
tests/train_batch_reference.py: the reference's torch expressions bit for bit where they are sums and products, float64 within 4 x the torch
formulation's own error where a pow or an interpolation is involved.

Shapes: 3 views of 37 x 53 (odd, and below the 128-cell error grid so several cells share a pixel) and one case at 160 x 144; 1, 255 and 257
rays per view (one lane, a ragged first workgroup, a second workgroup); 1 and 2 views per batch."""
import functools

import numpy as np
import pytest
import torch

from palettenerf_amd import rays as prays
from palettenerf_amd import scene, trainset
from tests import train_batch_reference as ref

pytestmark = pytest.mark.gpu
V = 3
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def stacks(H, W, C, D=16):
    """Host data of one scene, made once: an 8-bit stack (alpha exactly 0 and 255 on a quarter of the pixels each), a float stack that no 8-bit
    file could hold (alpha exactly 0 and 1 likewise; colours exactly 0, 1 and the sRGB knee planted), features, poses, intrinsics."""
    g = np.random.default_rng(H * 1000 + W + C)
    u8 = g.integers(0, 256, size=(V, H, W, C), dtype=np.uint8)
    f = g.random((V, H, W, C), dtype=F32)
    f[:, 0, :6, :3] = np.array([0.0, 1.0, 0.04045, np.nextafter(F32(0.04045), F32(0)), 0.5, 1e-6], F32)[None, :, None]
    if C == 4:
        kind = g.integers(0, 4, size=(V, H, W))
        u8[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, u8[..., 3]))
        f[..., 3] = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, f[..., 3]))
    feat = g.standard_normal((V, H, W, D), dtype=F32)
    poses = np.stack([scene.lookat_pose(azimuth_deg=az, elevation_deg=el) for az, el in ((45.0, 30.0), (170.0, 10.0), (-60.0, 55.0))]).astype(F32)
    return dict(u8=u8, f=f, feat=feat, poses=poses, intr=scene.intrinsics_from_fov(H, W))


def make_set(H, W, C, storage, N, feat=None, **kw):
    d = stacks(H, W, C)
    images = d["u8"] if storage == "uint8" else d["f"]
    feats = None if feat is None else torch.from_numpy(d["feat"]).to(feat)
    return trainset.TrainSet(images, d["poses"], d["intr"], H, W, N, feat_images=feats, storage=storage, **kw)


def decoded(ts):
    """The stored stack as the fp32 values the loader would hold: a uint8 stack through numpy's `astype(float32) / 255` on the host, as the loader
    does it (torch's division of a device tensor by a number multiplies by the reciprocal: not the same bits); fp16 converts exactly."""
    if ts.images.dtype == torch.uint8:
        return torch.from_numpy(ref.decode(ts.images.cpu().numpy())).to(ts.images.device)
    return ts.images.float()


def some_inds(cuda, H, W, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    inds = torch.randint(0, H * W, (B, N), generator=g)
    inds[:, 0] = H * W - 1                      # the last pixel of a view
    inds[:, -1] = 0
    return inds.to(cuda)


def views(cuda, B):
    return torch.tensor([V - 1, 0][:B], dtype=torch.int64, device=cuda)        # on the device, not monotone, the last view first


CASES = [(37, 53, 1, 1, "fp32", 4, torch.float32), (37, 53, 255, 1, "fp16", 4, torch.float16), (37, 53, 257, 1, "uint8", 4, torch.float32),
         (37, 53, 1, 2, "uint8", 3, torch.float16), (37, 53, 255, 2, "fp32", 3, torch.float32), (37, 53, 257, 2, "fp16", 3, torch.float16),
         (37, 53, 257, 2, "uint8", 4, None), (160, 144, 257, 2, "fp16", 4, torch.float16), (160, 144, 255, 1, "fp32", 3, None)]


@pytest.mark.parametrize("H,W,N,B,storage,C,feat", CASES)
def test_rays_and_gathers_are_bit_for_bit(cuda, H, W, N, B, storage, C, feat):
    ts = make_set(H, W, C, storage, N, feat)
    vi, inds = views(cuda, B), some_inds(cuda, H, W, B, N, N + B)
    o = ts._launch(vi, inds, want=("rays", "pixels", "gt_clip"))
    ro, rd = prays.rays_from_indices(ts.poses[vi], ts.intrinsics, H, W, inds)
    assert o["rays_o"].shape == (B, N, 3) and torch.equal(o["rays_o"], ro) and torch.equal(o["rays_d"], rd)
    assert o["pixels"].shape == (B, N, C) and torch.equal(o["pixels"], ref.collate_torch(decoded(ts), vi, inds))     # the reference's gather
    if storage == "uint8":
        assert torch.equal(ts.images, torch.from_numpy(stacks(H, W, C)["u8"]).to(cuda))                  # the bytes are held as they came
    else:
        assert torch.equal(o["pixels"], ref.collate_torch(ts.images, vi, inds).float())                  # gathered in the stored dtype, as -O does
    if feat is None:
        assert "gt_clip" not in o
    else:
        assert ts.feat_images.dtype == feat and torch.equal(o["gt_clip"], ref.collate_torch(ts.feat_images, vi, inds).float())
    out = ts.collate(vi)
    assert set(out) == {"H", "W", "rays_o", "rays_d", "inds", "images"} | ({"feat_images"} if feat is not None else set())
    assert out["images"].shape == (B, N, C) and out["inds"].shape == (B, N) and (out["H"], out["W"]) == (H, W)
    one = ts.collate(V - 1)                                              # a host int chooses the same view as the device index
    assert torch.equal(one["rays_o"][0, :, :], ts.poses[V - 1, :3, 3].expand(N, 3))


@pytest.mark.parametrize("storage", ["fp32", "fp16", "uint8"])
@pytest.mark.parametrize("N,B", [(1, 1), (255, 2), (257, 1)])
def test_blend_is_torchs_fp32_expression_bit_for_bit(cuda, storage, N, B):
    H, W = 37, 53
    ts = make_set(H, W, 4, storage, N)
    vi, inds = views(cuda, B), some_inds(cuda, H, W, B, N, 7 * N + B)
    inds[:, : min(N, 6)] = torch.arange(min(N, 6), device=cuda)          # the planted colours
    px = ref.collate_torch(decoded(ts), vi, inds)
    alpha = px[..., 3]
    if N > 1:
        assert bool((alpha == 0).any()) and bool((alpha == 1).any())
    per_ray = torch.rand(B, N, 3, device=cuda)
    for bg in (1, 0.25, torch.tensor([0.1, 0.7, 0.3], device=cuda), per_ray):
        got = ts._launch(vi, inds, bg=bg, want=("gt_rgb",))["gt_rgb"]
        want = ref.head_torch(px, bg)
        assert got.shape == (B, N, 3) and torch.equal(got, want), f"bg {bg if not torch.is_tensor(bg) else tuple(bg.shape)}"
    b = ts.batch(vi, bg_color=per_ray)
    assert torch.equal(b.gt_rgb, ref.head_torch(ref.collate_torch(decoded(ts), vi, b.inds), per_ray)) and b.gt_weights is None and b.gt_clip is None
    three = make_set(H, W, 3, storage, N)                                # no alpha: the colour itself, the background is not read
    got = three._launch(vi, inds, bg=per_ray, want=("gt_rgb", "pixels"))
    assert torch.equal(got["gt_rgb"], got["pixels"]) and three.batch(vi).bg_color == 1


@pytest.mark.parametrize("storage,C", [("fp32", 4), ("uint8", 4), ("fp16", 3)])
def test_linear_colour_is_within_four_times_torchs_own_error(cuda, storage, C):
    H, W, N, B = 37, 53, 257, 2
    ts = make_set(H, W, C, storage, N, color_space="linear")
    vi, inds = views(cuda, B), some_inds(cuda, H, W, B, N, 3)
    inds[:, :6] = torch.arange(6, device=cuda)
    bg = torch.rand(B, N, 3, device=cuda)
    got = ts._launch(vi, inds, bg=bg, want=("gt_rgb",))["gt_rgb"].cpu().numpy().astype(F64)
    px = ref.collate_torch(decoded(ts), vi, inds)
    exact = ref.blend_f64(px.cpu().numpy().astype(F64), bg.cpu().numpy().astype(F64), linear=True)
    E = np.abs(ref.head_torch(px, bg, linear=True)[..., :3].cpu().numpy().astype(F64) - exact).max()
    err = np.abs(got - exact).max()
    print(f"srgb_to_linear {storage} C={C}: kernel {err:.3g}, torch fp32 E {E:.3g}")
    assert E > 0 and err <= 4 * E


@functools.lru_cache(maxsize=None)
def guide_table(nb, S, normalised):
    g = np.random.default_rng(nb * 100 + S)
    hist = g.random((nb, S, S, S)).astype(F32)
    if normalised:
        hist = (hist / hist.sum(0, keepdims=True)).astype(F32)
    return hist


def guide_set(cuda, S):
    """A 3-channel fp32 set whose first view holds the colours the guide is checked at: exactly 0, exactly 1, bin nodes i / (S - 1), random."""
    H, W = 37, 53
    g = np.random.default_rng(S)
    img = g.random((V, H, W, 3), dtype=F32)
    flat = img[0].reshape(-1, 3)
    flat[0], flat[1], flat[2], flat[3] = 0.0, 1.0, (0.0, 1.0, 0.5), (1.0, 0.0, 1.0)
    flat[4:260] = (g.integers(0, S, size=(256, 3)) / (S - 1)).astype(F32)
    d = stacks(H, W, 3)
    ts = trainset.TrainSet(img, d["poses"], d["intr"], H, W, H * W)
    inds = torch.arange(H * W, device=cuda)[None]
    return ts, torch.zeros(1, dtype=torch.int64, device=cuda), inds


@pytest.mark.parametrize("nb,S", [(4, 32), (5, 32), (8, 32), (4, 8), (5, 8), (8, 8)])
def test_weight_guide_is_within_four_times_grid_samples_own_error(cuda, nb, S):
    ts, vi, inds = guide_set(cuda, S)
    for normalised in (False, True):
        hist = guide_table(nb, S, normalised)
        hw = torch.from_numpy(hist).to(cuda)[None]
        o = ts._launch(vi, inds, hist=hw, want=("gt_rgb",))
        rgb = o["gt_rgb"]
        assert torch.equal(rgb[0], ts.images[0].reshape(-1, 3))
        exact = ref.lut_f64(rgb.cpu().numpy().astype(F64), hist.astype(F64))
        E = np.abs(ref.lut_torch(rgb, hw).cpu().numpy().astype(F64) - exact).max()
        got = o["gt_weights"].cpu().numpy().astype(F64)
        err = np.abs(got - exact).max()
        print(f"guide nb={nb} S={S} normalised={normalised}: kernel {err:.3g}, torch grid_sample fp32 E {E:.3g}")
        assert got.shape == (1, 37 * 53, nb) and E > 0 and err <= 4 * E
        held = torch.from_numpy(np.ascontiguousarray(np.moveaxis(hist, 0, -1))).to(cuda).permute(3, 0, 1, 2)[None]    # as the reference holds it: [R,G,B,nb] permuted
        assert not held.is_contiguous() and torch.equal(ts._launch(vi, inds, hist=held, want=())["gt_weights"], o["gt_weights"])
        assert np.array_equal(got[0, 0], hist[:, 0, 0, 0].astype(F64))                  # colour 0: the first node alone
        assert np.array_equal(got[0, 1], hist[:, -1, -1, -1].astype(F64))               # colour 1: the upper corners are outside and count as zero
        if normalised:
            rows = np.abs(got.sum(-1) - 1).max()
            print(f"      rows sum to 1 within {rows:.3g}")
            assert rows <= 4 * E


def test_batch_gives_the_guide_only_to_a_model_that_has_one(cuda):
    ts, vi, _ = guide_set(cuda, 8)
    hw = torch.from_numpy(guide_table(5, 8, True)).to(cuda)[None]
    model = type("M", (), {"hist_weights": hw, "bg_radius": -1})()
    b = ts.batch(vi, model)
    assert b.gt_weights.shape == (1, 37 * 53, 5) and ts.batch(vi, type("M", (), {"bg_radius": -1})()).gt_weights is None
    exact = ref.lut_f64(b.gt_rgb.cpu().numpy().astype(F64), guide_table(5, 8, True).astype(F64))
    assert np.abs(b.gt_weights.cpu().numpy() - exact).max() <= 4 * np.abs(ref.lut_torch(b.gt_rgb, hw).cpu().numpy() - exact).max()


@pytest.mark.parametrize("N,B", [(1, 1), (255, 2), (257, 2)])
def test_error_map_update_is_torchs_scatter_bit_for_bit(cuda, N, B):
    H, W = 37, 53
    ts = make_set(H, W, 4, "fp16", N, error_map=True)
    ts.error_map.copy_(torch.rand(V, trainset.ERROR_CELLS, generator=torch.Generator().manual_seed(N)).to(cuda) + 0.01)
    want = ts.error_map.clone()
    vi = views(cuda, B)
    for rep in range(2):                                                   # two updates in a row on one stream
        b = ts.batch(vi)
        assert b.inds_coarse.shape == (B, N) and all(len(set(r)) == N for r in b.inds_coarse.tolist())     # multinomial without replacement
        loss = torch.rand(B, N, device=cuda)
        ts.update_error_map(b, loss)
        ref.error_map_torch(want, vi, b.inds_coarse, loss)
        assert torch.equal(ts.error_map, want), rep
    untouched = [v for v in range(V) if v not in vi.tolist()]
    assert untouched and all(int((ts.error_map[v] != want[v]).sum()) == 0 for v in untouched)
    first = torch.rand(V, trainset.ERROR_CELLS, generator=torch.Generator().manual_seed(N)).to(cuda) + 0.01
    assert all(torch.equal(ts.error_map[v], first[v]) for v in untouched) and not torch.equal(ts.error_map[vi[0]], first[vi[0]])
    out = ts.collate(vi)
    assert torch.equal(out["index"], vi) and out["inds_coarse"].shape == (B, N)


@pytest.mark.parametrize("mode", ["plain", "patch", "pairs", "error_map"])
@pytest.mark.parametrize("B", [1, 2])
def test_a_seed_selects_what_get_rays_selects(cuda, mode, B):
    H, W, N = 37, 53, 256
    kw = {"plain": {}, "patch": dict(patch_size=4), "pairs": dict(random_size=5), "error_map": dict(error_map=True)}[mode]
    ts = make_set(H, W, 4, "fp32", N, **kw)
    if ts.error_map is not None:
        ts.error_map.copy_(torch.rand(V, trainset.ERROR_CELLS, generator=torch.Generator().manual_seed(2)).to(cuda))
    vi = views(cuda, B)
    torch.manual_seed(123)
    want = ref.parent_batch(ts.poses, ts.intrinsics, H, W, N, ts.images, vi, error_map=ts.error_map, patch_size=kw.get("patch_size", 1),
                            random_size=kw.get("random_size", 0))
    after = torch.rand(4, device=cuda)
    torch.manual_seed(123)
    b = ts.batch(vi)
    assert torch.equal(torch.rand(4, device=cuda), after)                  # as many draws, in the same order
    assert torch.equal(b.inds, want["inds"]) and torch.equal(b.rays_o, want["rays_o"]) and torch.equal(b.rays_d, want["rays_d"])
    assert torch.equal(b.bg_color, want["bg_color"]) and torch.equal(b.gt_rgb, want["gt_rgb"])
    assert (b.inds_coarse is None) == ("inds_coarse" not in want) and (b.inds_coarse is None or torch.equal(b.inds_coarse, want["inds_coarse"]))


def test_a_pixel_id_past_the_image_is_clamped_to_the_last_pixel(cuda):
    H, W = 37, 53
    ts = make_set(H, W, 4, "fp16", 4, torch.float16)
    hw = torch.from_numpy(guide_table(4, 8, True)).to(cuda)[None]
    vi = views(cuda, 2)
    inds = torch.tensor([[H * W, H * W - 1, -1, 0]] * 2, dtype=torch.int64, device=cuda)
    o = ts._launch(vi, inds, bg=0.5, hist=hw, want=("rays", "pixels", "gt_rgb", "gt_clip"))
    for name, t in o.items():
        assert torch.equal(t[:, 0], t[:, 1]) and torch.equal(t[:, 2], t[:, 3]), name
    assert torch.equal(o["pixels"][:, 1], decoded(ts)[vi, H - 1, W - 1]) and torch.equal(o["gt_clip"][:, 1], ts.feat_images[vi, H - 1, W - 1].float())
    past = ts._launch(vi + V, inds, want=("pixels",))["pixels"]          # a view index past the stack: the last view
    assert torch.equal(past[0], decoded(ts)[V - 1].reshape(-1, 4)[[H * W - 1, H * W - 1, 0, 0]])


def palette_model(cuda, hist):
    from palettenerf_amd import network, raymarching, renderer
    torch.manual_seed(0)
    m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m.initialize_palette([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.8, 0.8, 0.7]], hist_weights=np.moveaxis(hist, 0, -1))
    m = m.to(cuda).train()
    with torch.no_grad():
        m.basis_color += 0.05                                                # off its origin: the anchor term is not zero
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m


def slab_set(cuda, N, **kw):
    """Three forward-facing views of the slab scene (configs[3]'s rig), RGBA fp16, 37 x 53."""
    H, W = 37, 53
    poses = []
    for i in range(V):
        a = 2 * np.pi * i / V
        p = np.eye(4, dtype=F32)
        p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3 * np.cos(a), 0.3 * np.sin(a), 1.5]
        poses.append(p)
    return trainset.TrainSet(stacks(H, W, 4)["f"], np.stack(poses), scene.intrinsics_from_fov(H, W, 0.9), H, W, N, storage="fp16", **kw)


RENDER = dict(dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4)
LAMBDAS = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_weight=0.05, lambda_palette=1e-3)


def test_train_step_is_the_reference_formulation_on_the_same_batch(cuda):
    from palettenerf_amd.train_loss import TERM_NAMES
    from tests.test_train_loss import torch_loss
    m = palette_model(cuda, guide_table(4, 8, True))
    assert tuple(m.hist_weights.shape) == (1, 4, 8, 8, 8)
    ts = slab_set(cuda, 257)
    torch.manual_seed(5)
    b = ts.batch(1, m)
    assert b.gt_weights.shape == (1, 257, 4) and b.bg_color.shape == (1, 257, 3)
    torch.manual_seed(6)
    pred, gt, loss, terms = trainset.train_step(m, b, RENDER, **LAMBDAS)
    assert pred.shape == (1, 257, 3) and gt is b.gt_rgb and terms["loss_ray"].shape == (1, 257) and set(TERM_NAMES) <= set(terms)
    torch.manual_seed(6)                                                    # the same perturbation of the march
    out = m.render(b.rays_o, b.rays_d, staged=False, bg_color=b.bg_color.reshape(-1, 3), perturb=True, force_all_rays=True, **RENDER)
    lam = dict(sparsity=LAMBDAS["lambda_sparsity"], offsets=LAMBDAS["lambda_offsets"], view_dep=LAMBDAS["lambda_view_dep"], smooth=0.0,
               weight=LAMBDAS["lambda_weight"], palette=LAMBDAS["lambda_palette"])
    gw = ref.lut_torch(b.gt_rgb, m.hist_weights)                            # the reference's guide on the same colours
    l_ref, t_ref = torch_loss(out, b.gt_rgb.reshape(-1, 3), lam, None, gw.reshape(-1, 4), m.basis_color, m.basis_color_origin)
    print(f"train_step loss {loss.item():.8g}, torch formulation {l_ref.item():.8g}")
    assert abs(loss.item() - l_ref.item()) <= 2e-6 * abs(l_ref.item())
    assert float(terms["loss_weight"]) > 0 and float(terms["loss_palette"]) > 0
    for name in TERM_NAMES[1:]:
        want = float(t_ref[name].detach()) if name in t_ref else 0.0
        print(f"      {name}: {float(terms[name]):.8g} vs {want:.8g}")
        assert abs(float(terms[name]) - want) <= 2e-6 * abs(want) + 1e-12, name
    loss.backward()
    assert m.basis_color.grad is not None and float(m.basis_color.grad.abs().max()) > 0


def test_two_train_epoch_steps_move_the_parameters(cuda):
    from palettenerf_amd import optim
    m = palette_model(cuda, guide_table(4, 8, True))
    ts = slab_set(cuda, 257, error_map=True)
    opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.1 ** min(it / 100, 1))
    before = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    torch.manual_seed(9)
    avg, step = trainset.train_epoch(m, ts, opt, sched, global_step=15, max_steps=2, render_kwargs=RENDER, generator=torch.Generator().manual_seed(1), **LAMBDAS)
    assert step == 17 and np.isfinite(avg) and avg > 0
    moved = [n for n, p in m.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert "basis_color" in moved and any(n.startswith("diff_net") for n in moved), moved
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert bool(torch.isfinite(ts.error_map).all()) and int((ts.error_map != 1).sum()) == 2 * 257      # two views' cells took their EMA


def test_train_epoch_on_a_nerf_model_updates_its_occupancy_first(cuda):
    """The NeRF stage (nerf/utils.py:527-536): force_all_rays=False, rays_gt = gt_rgb, the rgb_norm term; update_extra_state at global step 0."""
    from palettenerf_amd import network, optim
    torch.manual_seed(0)
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1.0, min_near=0.02).to(cuda).train()
    ts = slab_set(cuda, 257, error_map=True)
    opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    before = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    grid = m.density_grid.clone()
    avg, step = trainset.train_epoch(m, ts, opt, global_step=0, max_steps=2, render_kwargs=RENDER, lambda_sparse=1e-3)
    assert step == 2 and np.isfinite(avg) and avg > 0 and not torch.equal(m.density_grid, grid)
    assert any(n.startswith("color_net") and not torch.equal(p.detach(), before[n]) for n, p in m.named_parameters() if p.requires_grad)
    assert bool(torch.isfinite(ts.error_map).all()) and int((ts.error_map != 1).sum()) == 2 * 257
