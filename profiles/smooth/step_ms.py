"""What the smooth-loss block (palette/renderer.py:360-378) costs in a PaletteNeRF training step: the configs[3]-shaped step of
bench.make_training_step (4 096 rays, slab scene, dt_gamma 1/128, optim.Adam, the fused loss) with model.require_smooth_loss = True and
lambda_smooth = 4e-3, measured as bench.training_leg measures: wall ms per step over --steps steps after --warmup, and kernel ms and launches
per step from a torch-profiler trace of 10 further steps.  One JSON line on stdout.

    python profiles/smooth/step_ms.py                      # the fused block (pnr_palette_smooth_*)
    python profiles/smooth/step_ms.py --torch-smooth       # fused_train_smooth = False: the block as the reference writes it
    python profiles/smooth/step_ms.py --smooth-off         # require_smooth_loss = False: the step bench.py times
    python profiles/smooth/step_ms.py --tree ../parent     # the package of another (built) checkout, e.g. the parent commit

Legs that are compared run in one session on one machine, alternating, each twice; the spread between the two repeats of a leg is the
yardstick for a difference (profiles/smooth/README.md)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--smooth-off", action="store_true")
    ap.add_argument("--torch-smooth", action="store_true")
    ap.add_argument("--pred-clip", action="store_true", help="with the clip head (pred_clip, clip_dim 16, smooth_sigma_clip 0.5)")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--label", default="")
    ap.add_argument("--trace", action="store_true", help="add the trace's per-kernel totals (launches and us per step, by kernel name) to the line")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    import numpy as np
    import torch
    import palettenerf_amd
    from palettenerf_amd import network, optim, raymarching, renderer, scene
    from palettenerf_amd.train_loss import train_loss
    if not torch.cuda.is_available():
        raise SystemExit("step_ms.py measures on a GPU; none is visible")
    device = torch.device("cuda:0")
    kw = dict(pred_clip=True, smooth_sigma_clip=0.5) if a.pred_clip else {}
    m = network.PaletteNetwork(renderer.default_opt(test=False, **kw), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m = m.to(device).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(device))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.require_smooth_loss = not a.smooth_off
    m.fused_train_smooth = not a.torch_smooth      # (a checkout without the fused block ignores it)
    H, W = 756, 1008
    g = torch.Generator().manual_seed(0)
    poses = []
    for i in range(17):
        ang = 2 * np.pi * i / 17
        p = np.eye(4, dtype=np.float32)
        p[:3, 0], p[:3, 1], p[:3, 2] = [1, 0, 0], [0, -1, 0], [0, 0, -1]
        p[:3, 3] = [0.3 * np.cos(ang), 0.3 * np.sin(ang), 1.5]
        poses.append(p)
    ro_all, rd_all = scene.get_rays(torch.from_numpy(np.stack(poses)), scene.intrinsics_from_fov(H, W, 0.9), H, W)
    ro_all, rd_all = ro_all.to(device), rd_all.to(device)
    opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    torch.manual_seed(0)
    target = torch.rand(a.rays, 3, device=device)[None]
    inds_all = torch.randint(0, H * W, [64, a.rays], generator=g).to(device)
    lam = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_palette=1e-3)
    if not a.smooth_off:
        lam["lambda_smooth"] = 4e-3            # main_palette.py:86
    origin = (m.basis_color.detach() + 0.02).clone()

    def step(i):
        inds = inds_all[i % 64]
        ro, rd = ro_all[i % 17, inds][None], rd_all[i % 17, inds][None]
        opt.zero_grad(set_to_none=True)
        r = m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
        loss, info = train_loss(r, target, basis_color=m.basis_color, basis_color_origin=origin, **lam)
        loss.backward()
        opt.step()
        return info

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        info = step(a.warmup + i)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps * 1e3
    rec = {"label": a.label, "package": os.path.dirname(os.path.abspath(palettenerf_amd.__file__)), "smooth": not a.smooth_off,
           "fused_train_smooth": bool(not a.torch_smooth and not a.smooth_off and hasattr(m, "smooth_branch")), "pred_clip": a.pred_clip,
           "wall_ms_per_step": wall, "steps": a.steps, "rays_per_step": a.rays, "samples_per_step": int(m.step_counter[(m.local_step - 1) % 16, 0]),
           "loss_smooth_last": float(info["terms"][5])}
    from torch.profiler import ProfilerActivity, profile
    n = 10
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(n):
            step(a.warmup + a.steps + i)
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    if not kernels:
        raise SystemExit("the profiler recorded no kernel")
    rec["kernel_ms_per_step"] = sum(e.device_time for e in kernels) / n / 1e3
    rec["launches_per_step"] = len(kernels) / n
    hip = [e for e in kernels if "pnr::" in e.name[:12] or "_ZN3pnr" in e.name[:12]]
    rec["launches_hip_per_step"] = len(hip) / n
    rec["launches_torch_per_step"] = (len(kernels) - len(hip)) / n
    smooth = {}
    for e in kernels:
        if "k_palette_smooth" in e.name:
            key = e.name[e.name.index("k_palette_smooth"):].split("(")[0].split("E")[0]
            smooth[key] = smooth.get(key, 0.0) + e.device_time / n
    rec["smooth_kernels_us_per_step"] = smooth
    if a.trace:
        by_name = {}
        for e in kernels:
            key = e.name.split("(")[0][:96]
            c = by_name.setdefault(key, [0.0, 0.0])
            c[0] += 1 / n
            c[1] += e.device_time / n
        rec["kernels_per_step"] = {k: [round(v[0], 1), round(v[1], 1)] for k, v in sorted(by_name.items(), key=lambda kv: -kv[1][1])}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
