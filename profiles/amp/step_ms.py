"""The loss-scaled (-O) training step three ways: the configs[3]-shaped PaletteNeRF step of bench.make_training_step(fp16=True) -- 4 096 rays,
slab scene, dt_gamma 1/128, fp16 autocast, the fused loss -- with

    --leg a    torch.optim.Adam + torch.amp.GradScaler          (what bench.py's fp16 training leg runs)
    --leg b    optim.Adam       + torch.amp.GradScaler          (one Adam launch; torch's unscale_ pass and its found_inf read-back)
    --leg c    optim.Adam       + optim.GradScaler              (pnr_grad_check + pnr_adam_step_amp: no read-back)

One leg: --warmup + --steps steps timed by the host clock around a final synchronise with no profiler attached, then 10 further steps under
torch.profiler for the kernel sum and the launches per step (every kernel of the process, the C-ABI ones included), one JSON line.

    python profiles/amp/step_ms.py --all       # a, b, c, a, b, c: one fresh process per leg and repeat, on one device

The figures are in profiles/amp/README.md."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def run_leg(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from palettenerf_amd import network, optim, raymarching, renderer, scene
    from palettenerf_amd.train_loss import train_loss
    if not torch.cuda.is_available():
        raise SystemExit("step_ms.py measures on a GPU; none is visible")
    device = torch.device("cuda:0")
    m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m = m.to(device).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(device))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
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
    adam = torch.optim.Adam if a.leg == "a" else optim.Adam
    opt = adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    scaler = (optim.GradScaler if a.leg == "c" else torch.amp.GradScaler)("cuda")
    torch.manual_seed(0)
    target = torch.rand(a.rays, 3, device=device)[None]
    inds_all = torch.randint(0, H * W, [64, a.rays], generator=g).to(device)
    lam = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_palette=1e-3)
    origin = (m.basis_color.detach() + 0.02).clone()

    def step(i):
        inds = inds_all[i % 64]
        ro, rd = ro_all[i % 17, inds][None], rd_all[i % 17, inds][None]
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            r = m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
            loss, _ = train_loss(r, target, basis_color=m.basis_color, basis_color_origin=origin, **lam)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss = step(a.warmup + i)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / max(1, a.steps) * 1e3
    steps_taken = sorted({float(s["step"]) for s in opt.state_dict()["state"].values()})
    rec = {"leg": a.leg, "label": a.label, "optimizer": f"{adam.__module__}.Adam", "scaler": f"{type(scaler).__module__}.GradScaler", "steps": a.steps,
           "warmup": a.warmup, "rays_per_step": a.rays, "wall_ms_per_step": wall, "samples_per_step": int(m.step_counter[(m.local_step - 1) % 16, 0]),
           "loss_last": float(loss.detach()), "scale_last": scaler.get_scale(), "adam_steps_taken": steps_taken}
    from torch.profiler import ProfilerActivity, profile
    n = 10
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(n):
            step(a.warmup + a.steps + i)
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    rec["kernel_ms_per_step"] = sum(e.device_time for e in kernels) / n / 1e3
    rec["launches_per_step"] = len(kernels) / n
    mine = [e for e in kernels if "k_adam" in e.name or "k_grad_check" in e.name]
    tail = [e for e in kernels if "amp_update_scale" in e.name or "multi_tensor_apply" in e.name or "k_adam" in e.name or "k_grad_check" in e.name]
    rec["optimizer_hip_kernel_us_per_step"] = sum(e.device_time for e in mine) / n
    rec["scaler_and_optimizer_kernel_us_per_step"] = sum(e.device_time for e in tail) / n     # pnr's two, torch's foreach (multi_tensor_apply) and amp kernels
    rec["scaler_and_optimizer_launches_per_step"] = len(tail) / n
    counts = {}
    for e in tail:
        short = next(t for t in ("k_adam", "k_grad_check", "amp_update_scale", "multi_tensor_apply") if t in e.name)
        counts[short] = counts.get(short, 0) + 1
    rec["scaler_and_optimizer_launches_by_kernel"] = {k: v / n for k, v in sorted(counts.items())}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("a", "b", "c"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not a.all:
        if not a.leg:
            ap.error("--leg or --all")
        return run_leg(a)
    for rep in range(1, a.repeats + 1):
        for leg in "abc":           # alternating: a difference between legs is judged against the difference between a leg's own repeats
            subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--label", f"{leg}_{rep}", "--steps", str(a.steps), "--warmup", str(a.warmup),
                            "--rays", str(a.rays)], check=True, timeout=300)


if __name__ == "__main__":
    main()
