"""Parity at BASELINE.json's full size (800x800 = 640 000 rays, scene S0) through size-independent properties and
checksums: the oracle needs ~40 s of CPU for this march, so its per-ray counts are pinned here by constants computed
once in the build container (oracle.march_rays_train on the same rays; see the comment next to each constant)."""
import os
import zlib

import numpy as np
import pytest
import torch

from palettenerf_amd import network, raymarching, scene

pytestmark = pytest.mark.gpu

# oracle.march_rays_train(800x800 S0 rays, bound 2, dt_gamma 0, max_steps 1024): counter, #rays with samples, max count, crc32(counts)
ORACLE_COUNTER = 63001854
ORACLE_HITTING_RAYS = 354841
ORACLE_MAX_COUNT = 509
ORACLE_COUNTS_CRC32 = 2971143974
RAYS_D_CRC32, RAYS_O_CRC32 = 540470127, 1262356950  # the deterministic (float64 -> float32) ray generator gives these bits on any host


@pytest.fixture(scope="module")
def frame800(cuda):
    grid = torch.from_numpy(scene.brick_density_grid()).to(cuda)
    bitfield = raymarching.packbits(grid, 0.5)
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(800, 800), 800, 800)
    assert zlib.crc32(rd[0].numpy().tobytes()) == RAYS_D_CRC32 and zlib.crc32(ro[0].numpy().tobytes()) == RAYS_O_CRC32
    return grid, bitfield, ro[0].to(cuda).contiguous(), rd[0].to(cuda).contiguous()


def test_full_frame_training_march_counts_and_structure(cuda, frame800):
    grid, bitfield, ro, rd = frame800
    N = ro.shape[0]
    aabb = torch.tensor([-2, -2, -2, 2, 2, 2], dtype=torch.float32, device=cuda)
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    M = 64 * 1024 * 1024  # mean_count path: M rows (2 GB of staging), nothing is dropped since counter < M
    xyzs, dirs, deltas, rays = raymarching.march_rays_train(ro, rd, 2.0, bitfield, 2, 128, nears, fars, counter, M - 128, False, 128, False, 0.0, 1024)
    assert xyzs.shape[0] == M
    counts = rays[:, 2].cpu().numpy()
    assert counter.cpu().tolist() == [ORACLE_COUNTER, N]
    assert int((counts > 0).sum()) == ORACLE_HITTING_RAYS and int(counts.max()) == ORACLE_MAX_COUNT
    assert zlib.crc32(counts.astype(np.int32).tobytes()) == ORACLE_COUNTS_CRC32          # every per-ray count equals the oracle's
    # structure: row n is ray n, offsets are the exclusive prefix sum of the counts
    assert torch.equal(rays[:, 0], torch.arange(N, dtype=torch.int32, device=cuda))
    assert torch.equal(rays[:, 1].long(), torch.cumsum(rays[:, 2].long(), 0) - rays[:, 2].long())
    m = ORACLE_COUNTER
    assert bool((deltas[:m, 0] > 0).all()) and bool((deltas[m:m + 4096] == 0).all())
    # every emitted sample lies in an occupied cell of the cascade the kernel chose for it
    p = xyzs[:m]
    mx = p.abs().amax(dim=1)
    level = (torch.frexp(mx).exponent.clamp(min=0, max=1)).long()  # dt is constant and small: the level comes from the position
    mb = torch.minimum(torch.exp2(level.float()), torch.tensor(2.0, device=cuda))[:, None]
    cell = (0.5 * (p / mb + 1) * 128).clamp(0, 127).int()
    index = level * 128 ** 3 + raymarching.morton3D(cell).long()
    occ = (bitfield[index // 8].int() >> (index % 8).int()) & 1
    assert bool(occ.all())
    # directions are the rays' own, repeated count times
    ray_of_row = torch.repeat_interleave(torch.arange(N, device=cuda), rays[:, 2].long())
    assert torch.equal(dirs[:m], rd[ray_of_row])


def test_full_frame_native_loop_equals_reference_style_loop(cuda, frame800):
    grid, bitfield, ro, rd = frame800
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(grid)
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.count_rendered = True
    out = {}
    for mode in ("compat", "native"):
        m.march_mode = mode
        m.fused_field = mode == "native"
        with torch.no_grad():
            out[mode] = m.render(ro[None], rd[None], perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    a, b = out["compat"], out["native"]
    assert int(a["rendered"].item()) == int(b["rendered"].item())  # same schedule, same compaction, same samples
    assert 9_000_000 < int(b["rendered"].item()) < 10_500_000
    assert float((a["image"] - b["image"]).abs().max()) < 2e-5
    assert float((a["weights_sum"] - b["weights_sum"]).abs().max()) < 2e-5
    assert scene.psnr(a["image"], b["image"]) > 90.0
    fin = torch.isfinite(a["depth"])
    assert torch.equal(fin, torch.isfinite(b["depth"])) and float((a["depth"][fin] - b["depth"][fin]).abs().max()) < 1e-4
    # idempotence: rendering the same frame twice gives bit-identical results (no atomics on the inference path)
    with torch.no_grad():
        c = m.render(ro[None], rd[None], perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
    assert torch.equal(b["image"], c["image"]) and torch.equal(b["weights_sum"], c["weights_sum"])


def test_full_size_grid_encode_linearity_and_checksum(cuda):
    """Hash-grid forward at B = 2^20: linear in the table (f(a T1 + b T2) = a f(T1) + b f(T2) up to rounding) and
    permutation-equivariant in the samples."""
    from palettenerf_amd import gridencoder
    g = torch.Generator(device="cpu").manual_seed(3)
    enc = gridencoder.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096).to(cuda)
    B = 1 << 20
    x = torch.rand(B, 3, generator=g).to(cuda)
    T1 = (torch.rand(enc.embeddings.shape, generator=g) - 0.5).to(cuda)
    T2 = (torch.rand(enc.embeddings.shape, generator=g) - 0.5).to(cuda)
    f = lambda T: gridencoder.grid_encode(x, T, enc.offsets, enc.per_level_scale, 16, False, 0, False)
    y1, y2, y12 = f(T1), f(T2), f(0.5 * T1 - 2.0 * T2)
    assert float((y12 - (0.5 * y1 - 2.0 * y2)).abs().max()) < 2e-6
    perm = torch.randperm(B, generator=g).to(cuda)
    yp = gridencoder.grid_encode(x[perm].contiguous(), T1, enc.offsets, enc.per_level_scale, 16, False, 0, False)
    assert torch.equal(yp, y1[perm])


def test_garden_video_frame_native_equals_reference_style_loop(cuda):
    """BASELINE configs[4] at its full size on one GPU: one pose of the 120-pose garden path (1297 x 840 = 1.09 M rays, PaletteNeRF,
    dt_gamma = 1/128, scene S2) through the device-driven loop against the host-driven loop with torch MLPs and the reference's seven
    composites (size-independent properties: same samples, same maps); then the 8-way tile sharding of the same frame reassembles it."""
    from palettenerf_amd import dist as pdist, rays as prays, renderer
    from palettenerf_amd.fused import tile_ray_order
    H, W = scene.GARDEN_H, scene.GARDEN_W
    opt = renderer.default_opt()
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.garden_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.count_rendered = True
    pose = torch.from_numpy(scene.garden_orbit_pose(17)[None]).to(cuda)
    ro, rd = prays.rays_from_indices(pose, scene.garden_intrinsics(), H, W, None)
    kw = dict(perturb=False, dt_gamma=1.0 / 128, max_steps=1024, T_thresh=1e-4, gui_mode=False)
    out = {}
    for mode in ("compat", "native"):
        m.march_mode = mode
        m.fused_field = mode == "native"
        with torch.no_grad():
            out[mode] = m.render(ro, rd, **kw)
    a, b = out["compat"], out["native"]
    na, nb_ = int(a["rendered"].sum()), int(b["rendered"].sum())
    # same schedule and compaction; the two loops evaluate sigma with different roundings (rocBLAS fp32 GEMMs vs the fused split-fp16 field),
    # so a handful of the 31 M samples fall on the other side of the T < 1e-4 termination test
    assert na > 5_000_000 and abs(na - nb_) <= 1e-5 * na, (na, nb_)
    for k in ("image", "weights_sum", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
        assert float((a[k] - b[k]).abs().max()) < 1e-4, k
    assert scene.psnr(a["image"], b["image"]) > 80.0
    fin = torch.isfinite(a["depth"])
    assert torch.equal(fin, torch.isfinite(b["depth"])) and float((a["depth"][fin] - b["depth"][fin]).abs().max()) < 1e-4
    hit = float((b["weights_sum"] > 0.5).float().mean())
    assert 0.3 < hit <= 1.0   # the ground slab and the object fill a large part of every view of the path
    # the 8-GPU split of this frame on one GPU: every tile shard rendered on its own (tile-ordered alive list, as bench.py does) gives its
    # pixels of the full frame bit for bit -- per-ray results do not depend on which rays share a launch
    full = b["image"][0]
    n_total = 0
    for rank in range(8):
        idx, _ = pdist.shard_indices(H, W, rank, 8)
        idx = idx.to(cuda)
        m._fused.ray_order = tile_ray_order(idx.cpu(), W, 8).to(cuda)
        with torch.no_grad():
            r = m.render(ro[:, idx].contiguous(), rd[:, idx].contiguous(), **kw)
        assert torch.equal(r["image"][0], full[idx])
        n_total += int(r["rendered"].sum())
    m._fused.ray_order = None
    # (march-emitted samples depend on the n_step schedule, which follows each launch's own N / n_alive: samples marched for a ray after it
    # terminated inside a group are counted but never composited -- the pixels above are what must agree)
    assert abs(n_total - int(b["rendered"].sum())) < 0.01 * n_total


def test_palette_frame_800_native_equals_reference_style_loop(cuda, frame800):
    """BASELINE configs[2] at full size: the 800x800 PaletteNeRF frame (all seven composited maps) through the device-driven loop against the
    host-driven loop with torch MLPs and the reference's seven composites; then the same with a RegionEdit active (inside the fused epilogue)."""
    from palettenerf_amd import renderer
    grid, bitfield, ro, rd = frame800
    opt = renderer.default_opt()
    m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(grid)
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.count_rendered = True
    kw = dict(perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4, gui_mode=False)

    def both():
        out = {}
        for mode in ("compat", "native"):
            m.march_mode, m.fused_field = mode, mode == "native"
            with torch.no_grad():
                out[mode] = m.render(ro[None], rd[None], **kw)
        return out["compat"], out["native"]

    a, b = both()
    na, nb_ = int(a["rendered"].sum()), int(b["rendered"].sum())
    assert 9_000_000 < nb_ < 10_500_000 and abs(na - nb_) <= 1e-5 * na
    for k in ("image", "weights_sum", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"):
        assert float((a[k] - b[k]).abs().max()) < 1e-4, k
    assert scene.psnr(a["image"], b["image"]) > 85.0
    m.edit = renderer.RegionEdit(opt)
    m.edit.update_cent(mean_xyz=torch.tensor([0.2, 0.1, -0.1], device=cuda))
    m.edit.update_std(std_xyz=0.3)
    m.edit.update_delta_hsv(m.basis_color.data.clamp(0, 1), (m.basis_color.data * 0.5 + 0.3).flip(0).clamp(0, 1))
    c, d = both()
    assert float((c["image"] - d["image"]).abs().max()) < 1e-4 and float((c["image"] - a["image"]).abs().max()) > 1e-2   # the edit is visible, and identical
    assert d["iterations"] == b["iterations"]                     # the edited frame takes the same device-driven loop, launch for launch


def test_palette_training_step_at_config3_size(cuda):
    """BASELINE configs[3] shape: one PaletteNeRF training step on 4096 rays of the forward-facing slab scene (dt_gamma 1/128, ~0.6 M samples) --
    the fused training path (one-launch MLP stacks, level-major encoder hand-off, fused colour-basis shade, frozen-density kernel, binned table
    gradient) against the same step on plain torch modules + the drop-in operators; then the one-launch Adam against torch.optim.Adam on those
    gradients."""
    import copy
    from palettenerf_amd import mlp, optim, renderer
    torch.manual_seed(0)
    m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m = m.to(cuda).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    H, W = 756, 1008
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]
    ro, rd = scene.get_rays(torch.from_numpy(pose)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    inds = torch.randint(0, H * W, [4096])
    ro, rd = ro[:, inds].to(cuda), rd[:, inds].to(cuda)
    target = torch.rand(4096, 3, device=cuda)

    def step(fused):
        mlp.enabled = fused
        m.fused_train_shade = m.fused_train_density = fused
        for p in m.parameters():
            p.grad = None
        r = m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=False, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
        loss = ((r["image"][0] - target) ** 2).mean() + 1e-3 * r["omega_sparsity"].mean() + 1e-2 * r["offsets_norm"].mean() + ((r["direct_rgb"][0] - target) ** 2).mean()
        loss.backward()
        return float(loss), int(m.step_counter[(m.local_step - 1) % 16, 0]), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    try:
        l_ref, n_ref, g_ref = step(False)
        l_fus, n_fus, g_fus = step(True)
    finally:
        mlp.enabled = True
    assert n_ref == n_fus > 400_000                      # the march does not depend on the field path
    assert abs(l_ref - l_fus) < 2e-5 * max(1.0, abs(l_ref))
    assert set(g_ref) == set(g_fus) and "encoder.embeddings" not in g_fus and "encoder_palette.embeddings" in g_fus    # geometry frozen (sigma detached)
    for name in g_ref:
        scale = float(g_ref[name].abs().max())
        # rounds 1-3 allowed 3e-3 of the largest entry; measured (profiles/r04_grad_tolerance.txt): 2.3e-8 ... 1.9e-6.  The torch path is fp32 GEMMs; the
        # fused path's MLP launches use split-fp16 products (22-bit, fp32 accumulation; pnr.h: pnr_mlp_*) forward and backward, everything else is fp32
        # in another summation order.  Bound: 4 x the worst measurement, rounded up.
        assert float((g_ref[name] - g_fus[name]).abs().max()) <= 1e-5 * scale + 1e-12, name
    # optimiser: same gradients, two identical models, one step each
    m2 = copy.deepcopy(m)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15).step()
    optim.Adam(m2.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15).step()
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n


def test_palette_two_stage_training_converges(cuda):
    """A short version of profiles/train_palette.py (configs[3]'s recipe: NeRF stage -> checkpoint -> PaletteNetwork + palette -> PaletteTrainer's loss):
    the PaletteNeRF stage must lift the held-out PSNR from its initial ~8 dB to above 28 dB within 400 steps."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_palette.py")
    spec = importlib.util.spec_from_file_location("train_palette", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    log = mod.main(["--steps", "400", "--nerf-steps", "400", "--log-every", "200", "--res", "0.125"])
    assert log[0][1] < 15.0 and log[-1][1] > 28.0, log


@pytest.mark.gpu
def test_bench_line_with_frames_in_flight_over_rccl(cuda):
    """`bench.py --main-frames-in-flight 2` through the RCCL path on one GPU (PNR_BENCH_FORCE_DIST: a one-rank communicator): two render threads, their
    all-gathers issued in frame order (dist.OrderedGather), one JSON line whose sample count equals the plain run's on the same camera path."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PNR_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    common = [sys.executable, os.path.join(root, "bench.py"), "--full", "--res", "200", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--no-extras"]
    lines = []
    for extra in ([], ["--main-frames-in-flight", "2"]):
        out = subprocess.run(common + extra, env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads(out.stdout.strip().splitlines()[-1]))
    plain, piped = lines
    assert plain["config"]["frames_in_flight"] == 1 and piped["config"]["frames_in_flight"] == 2
    assert piped["config"]["rccl_ranks"] == 1 and piped["config"]["gathered_floats_per_ray"] == 5
    assert piped["config"]["rendered_samples_per_step"] == plain["config"]["rendered_samples_per_step"]
    assert piped["value"] > 0 and "note_frames_in_flight" in piped["roofline"]


@pytest.mark.gpu
def test_bench_default_line_for_more_than_one_rank_over_rccl(cuda):
    """The N > 1 default of bench.py -- configs[4], ONE garden frame's rays sharded in 32 x 32 tiles, one all-gather per frame, strong scaling -- over
    a one-rank RCCL communicator (PNR_BENCH_FORCE_DIST=1 + --dist-default): the parsed line names configs[4], carries the ranks' shard render ms, the
    all-gather by HIP events and the single-GPU time of the same frame, and extra.weak holds the weak-scaling leg."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PNR_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29549")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--dist-default", "--steps", "4", "--warmup", "2", "--extra-steps", "5", "--res", "200", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    cfg = line["config"]
    assert line["scaling"] == "strong" and line["n_gpus"] == 1 and cfg["rccl_ranks"] == 1 and cfg["defaulted_for_ranks"] is True
    assert cfg["workload"].startswith("configs[4]") and "840x1297" in cfg["workload"] and cfg["rays_per_step"] == 840 * 1297
    assert cfg["gathered_floats_per_ray"] == 24 and cfg["all_gather_bytes_per_rank"] == 840 * 1297 * 24 * 4
    assert len(cfg["shard_render_ms_per_rank"]) == 1 and 0 < cfg["shard_render_ms_per_rank"][0] < line["ms_per_step"] * 1.5
    assert cfg["all_gather_ms"] > 0 and cfg["single_gpu_ms_per_step"] > 0
    assert 0.5 < cfg["strong_speedup_vs_single_gpu_in_this_job"] < 1.5            # one rank: the "split" is the whole frame
    assert line["value"] > 0 and cfg["rendered_samples_per_step"] == cfg["single_gpu_samples_per_step"]
    weak = line["extra"]["weak"]
    assert weak["workload"].startswith("configs[1]") and weak["pipelined"]["value"] > 0 and weak["gathered_floats_per_ray"] == 5
    # round 6: the numbers a strong-scaling curve is read from sit at the top level, and the roofline object stands on its own -- a fraction of a peak that can
    # bound the kernel (the interleaved PaletteNeRF lookup is served on-die: L2, not HBM) next to HBM-side traffic MEASURED in this run (two single-GPU PMC child passes)
    for k in ("strong_speedup_vs_single_gpu_in_this_job", "single_gpu_ms_per_step", "shard_render_ms_per_rank", "all_gather_ms"):
        assert line[k] == cfg[k]
    roof = line["roofline"]
    assert roof["bound"] in ("hbm", "l2") and 0 < roof["frac"] <= 1.0, roof
    assert roof["traffic"] is not None and roof["traffic"] > 0, roof.get("traffic_source")
    assert 0 < roof["hbm_frac_of_measured_traffic"] <= 1.0
    if roof["bound"] == "l2":
        assert roof["algorithmic_over_hbm_peak"] > 1.0 and roof["peak"] > 8000.0
    assert "ceilings_source" in roof["l2_bound"]


def test_headline_crop_against_the_live_oracle_and_its_committed_digest(cuda, golden_dir):
    """The comparison bench.py's `parity` block makes, as a test: the centre 400 x 400 crop of pose 0 of the configs[1] frame (800 x 800, S0,
    -m nerf, density_scale 100) through the device-driven native loop (split-fp16 field: the headline's arithmetic)
      (a) against the oracle run LIVE on the same rays on this host (per pixel: 1e-5; measured 5.4e-7), and
      (b) against tests/golden/crop400.npz, the oracle's digest committed from the build container (rendered-sample count exact; 8 x 8 block
          means of image and alpha to 1e-5), so that an oracle that drifted between the container and this box cannot hide a kernel change."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_crop400", os.path.join(golden_dir, "gen_crop400.py"))
    gc400 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gc400)
    fx = np.load(os.path.join(golden_dir, "crop400.npz"))
    import bench
    from palettenerf_amd.fused import NeRFFieldFused
    args = bench.parse(["--no-extras"])
    m = bench.build_model(args, cuda, "nerf")
    assert m.march_mode == "native" and isinstance(m._fused, NeRFFieldFused) and m._fused.precision == 1
    ro, rd = gc400.crop_rays()
    with torch.no_grad():
        g = m.render(ro.to(cuda), rd.to(cuda), perturb=False, dt_gamma=0.0, max_steps=1024, T_thresh=1e-4)
    img, ws = g["image"][0].cpu().numpy(), g["weights_sum"].cpu().numpy()
    # (b) the committed digest
    assert int(g["rendered"].sum()) == int(fx["rendered"])                       # march + termination: the same samples as the oracle rendered
    np.testing.assert_allclose(gc400.block_means(img), fx["image_block_means"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(gc400.block_means(np.repeat(ws[:, None], 3, 1))[..., 0], fx["alpha_block_means"], rtol=0, atol=1e-5)
    # (a) the live oracle, per pixel
    oimg, ows, on = gc400.oracle_crop(threads=min(16, os.cpu_count() or 1))
    assert on == int(fx["rendered"])
    np.testing.assert_allclose(gc400.block_means(oimg), fx["image_block_means"], rtol=0, atol=2e-6)      # this host's oracle == the container's
    assert float(np.abs(img - oimg).max()) <= 1e-5 and float(np.abs(ws - ows).max()) <= 1e-5
    assert scene.psnr(torch.from_numpy(img), torch.from_numpy(oimg)) > 100.0


@pytest.mark.parametrize("name", ["crop400_palette", "crop256_garden"])
def test_palette_crops_against_the_live_oracle_and_their_committed_digests(cuda, golden_dir, name):
    """configs[2] (800 x 800 PaletteNeRF frame, S0; centre 400 x 400) and configs[4] (1297 x 840 garden frame, S2, dt_gamma 1/128; centre 256 x 256)
    through the device-driven native loop with the split-fp16 palette field -- the arithmetic the bench legs time -- against
      (b) tests/golden/<name>.npz, the oracle's digest committed from the build container (tests/golden/gen_crops_palette.py): rendered-sample count
          exact, 8 x 8 block means of image / alpha / view_dep_rgb / basis_rgb / basis_acc to 1e-5, and
      (a) the oracle run LIVE on this host on the same rays, per pixel to 1e-5 (the colour contract is 1e-4).
    Before round 5 the full-size PaletteNeRF images were only compared native vs compat -- HIP against HIP."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_crops_palette", os.path.join(golden_dir, "gen_crops_palette.py"))
    gcp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gcp)
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    import bench
    from palettenerf_amd.fused import PaletteFieldFused
    args = gcp.case_args(name)
    c = gcp.CASES[name]["crop"]
    m = bench.build_model(args, cuda, "palette")
    assert m.march_mode == "native" and isinstance(m._fused, PaletteFieldFused) and m._fused.precision == 1
    ro, rd = gcp.crop_rays(name)
    with torch.no_grad():
        g = m.render(ro.to(cuda), rd.to(cuda), perturb=False, dt_gamma=args.wl["dt_gamma"], max_steps=1024, T_thresh=1e-4, gui_mode=False)
    # (b) the committed digest.  The march itself is bit-exact (ray-point counts: tests/test_gpu_ops.py, test_gpu_reference_kernels.py); `rendered` also counts
    # on WHEN a ray's transmittance falls below T_thresh, a comparison of floats that the two arithmetics (split-fp16 MFMA here, fp32 BLAS in the oracle)
    # decide differently for a handful of rays whose T sits within 1e-6 of the threshold: the lego crops match exactly, the garden crop (dt_gamma 1/128,
    # 1.9 M samples) by 4 samples (measured on three boxes, rounds 5-6).  Such a ray ends one sample apart: at most T_thresh = 1e-4 of one sample's colour.
    # Slack = twice the measured 4; the per-pixel bound on those rays is north_star's colour contract, 1e-4 (measured 2.2e-5 on alpha, 3.8e-6 on rgb).
    slack = 0 if name == "crop400_palette" else 8
    assert abs(int(g["rendered"].sum()) - int(fx["rendered"])) <= slack
    assert int((g["weights_sum"] > 0).sum()) == int(fx["hit_rays"])
    dg = gcp.digest(g, c)
    for k, v in dg.items():
        np.testing.assert_allclose(v, fx[k], rtol=0, atol=1e-5, err_msg=k)
    # (a) the live oracle, per pixel
    o = gcp.oracle_crop(name, threads=min(16, os.cpu_count() or 1))
    assert int(o["rendered"].item()) == int(fx["rendered"])
    for k, v in gcp.digest(o, c).items():
        np.testing.assert_allclose(v, fx[k], rtol=0, atol=2e-6, err_msg="oracle on this host vs the container: " + k)
    for k in gcp.MAPS + ("weights_sum",):
        a, b = g[k].detach().cpu().reshape(c * c, -1), o[k].reshape(c * c, -1)
        d = (a - b).abs().max(dim=1).values
        assert int((d > 1e-5).sum()) <= slack and float(d.max()) <= (1e-5 if slack == 0 else 1e-4), (k, float(d.max()), int((d > 1e-5).sum()))
    assert scene.psnr(g["image"].cpu().reshape(-1, 3), o["image"].reshape(-1, 3)) > 100.0
