"""What the weights' average costs a trainer that updates it after EVERY optimiser step (torch_ema's documented loop; the reference's own trainer
updates once per epoch -- see README.md here): the configs[3]-shaped PaletteNeRF -O step of profiles/amp/step_ms.py's leg c -- 4 096 rays, slab
scene, dt_gamma 1/128, fp16 autocast, the fused loss, optim.Adam + optim.GradScaler -- with

    --leg a    the parent commit's step, no average             (needs --parent-tree: a built checkout of the parent commit)
    --leg b    this build's step + the control's three torch expressions per parameter tensor after it   (what a torch_ema user pays)
    --leg c    this build's step + optim.ExponentialMovingAverage.update()                 (pnr_ema_update: one launch)
    --leg e    this build's step, no average
    --leg swap store + copy_to + restore (torch_ema's way: a clone and two copies of every tensor) against two swap() on the same model,
               device events, alternating
(There is no leg d: the update folded into the optimiser's launch was measured on a build that had it and was not kept -- README.md here.)

One leg, plain: --warmup + --steps steps timed by the host clock around a final synchronise, no profiler attached: wall ms per step.
One leg, --traced (run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python step_ms.py --leg X --traced`): the
same steps; the parent process then reads DIR's kernel trace and reports the kernel sum and the launches per step over the timed steps (a step =
the dispatches from one k_grad_check to the next: every step has exactly one).

    python profiles/ema/step_ms.py --all [--parent-tree DIR] [--out DIR]     # every leg plain and traced, legs alternating, --repeats times

The figures are in profiles/ema/README.md."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))


def run_leg(a):
    sys.path.insert(0, os.path.abspath(a.parent_tree) if a.leg == "a" else ROOT)
    import numpy as np
    import torch
    import palettenerf_amd
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
    params = list(m.parameters())
    if a.leg == "swap":
        return run_swap(a, m, params, optim, torch)
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
    scaler = optim.GradScaler("cuda")
    torch.manual_seed(0)
    target = torch.rand(a.rays, 3, device=device)[None]
    inds_all = torch.randint(0, H * W, [64, a.rays], generator=g).to(device)
    lam = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_palette=1e-3)
    origin = (m.basis_color.detach() + 0.02).clone()

    shadows, updates = [p.clone().detach() for p in params], [0]

    def control_update():          # torch_ema's update, written out (tests/ema_reference.py)
        updates[0] += 1
        one_minus_decay = 1.0 - min(0.95, (1 + updates[0]) / (10 + updates[0]))
        with torch.no_grad():
            for s_param, param in zip(shadows, params):
                tmp = s_param - param
                tmp.mul_(one_minus_decay)
                s_param.sub_(tmp)

    after_step = None
    if a.leg == "b":
        after_step = control_update
    elif a.leg == "c":
        ema = optim.ExponentialMovingAverage(params, 0.95)
        after_step, shadows = ema.update, ema.shadow_params

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
        if after_step is not None:
            after_step()
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
    checksum = float(sum(s.double().sum() for s in shadows)) if a.leg in "bc" else None       # (the run is not reproducible across processes: perturb, atomics)
    rec = {"leg": a.leg, "label": a.label, "traced": bool(a.traced), "tree": os.path.dirname(os.path.dirname(os.path.abspath(palettenerf_amd.__file__))),
           "steps": a.steps, "warmup": a.warmup, "rays_per_step": a.rays, "tracked_tensors": len(params), "tracked_elements": sum(p.numel() for p in params),
           "loss_last": float(loss.detach()), "scale_last": scaler.get_scale(), "adam_steps_taken": steps_taken, "shadow_checksum": checksum}
    rec["wall_ms_per_step_traced" if a.traced else "wall_ms_per_step"] = wall
    print(json.dumps(rec), flush=True)


def run_swap(a, m, params, optim, torch):
    ema = optim.ExponentialMovingAverage(params, 0.95)
    with torch.no_grad():
        for s in ema.shadow_params:
            s.mul_(0.9)

    def torch_ema_way():
        collected = [p.clone() for p in params]                       # store
        for s, p in zip(ema.shadow_params, params):                   # copy_to
            p.data.copy_(s.data)
        for c, p in zip(collected, params):                           # restore
            p.data.copy_(c.data)

    def two_swaps():
        ema.swap()
        ema.swap()

    def ours_store_way():
        ema.store(), ema.copy_to(), ema.restore()

    times = {"store_copy_to_restore_torch_ema": [], "store_copy_to_restore_foreach": [], "two_swaps": []}
    fns = {"store_copy_to_restore_torch_ema": torch_ema_way, "store_copy_to_restore_foreach": ours_store_way, "two_swaps": two_swaps}
    for rep in range(a.repeats * 10 + 2):
        for name, fn in fns.items():                                  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:                                              # two warm-up rounds
                times[name].append((e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6))
    rec = {"leg": "swap", "label": a.label, "tracked_tensors": len(params), "tracked_bytes": 4 * sum(p.numel() for p in params), "rounds": a.repeats * 10}
    for name, ts in times.items():
        dev, host = sorted(t[0] for t in ts), sorted(t[1] for t in ts)
        rec[name] = {"device_us_median": dev[len(dev) // 2], "device_us_min": dev[0], "device_us_max": dev[-1], "host_us_median": host[len(host) // 2]}
    print(json.dumps(rec), flush=True)


def trace_summary(out_dir, warmup, steps):
    """Kernel sum and launches per step over the timed steps from rocprofv3's per-dispatch kernel trace."""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"trace_error": "no *kernel_trace.csv under " + out_dir, "files": sorted(os.listdir(out_dir))}
    with open(files[0], newline="") as f:
        rows = list(csv.reader(f))
    header = [h.strip().lower() for h in rows[0]]
    try:
        k_name = next(i for i, h in enumerate(header) if h == "kernel_name")
        k_start = next(i for i, h in enumerate(header) if h.startswith("start"))
        k_end = next(i for i, h in enumerate(header) if h.startswith("end"))
    except StopIteration:
        return {"trace_error": "unexpected columns", "header": rows[0]}
    disp = sorted(((int(r[k_start]), int(r[k_end]), r[k_name]) for r in rows[1:] if len(r) > max(k_name, k_start, k_end)), key=lambda d: d[0])
    marks = [i for i, d in enumerate(disp) if "k_grad_check" in d[2]]
    c = len(marks) // (warmup + steps)                                 # k_grad_check launches per step (one per 32 tensors with a gradient)
    if c < 1 or len(marks) != c * (warmup + steps):
        return {"trace_error": f"{len(marks)} k_grad_check dispatches for {warmup + steps} steps"}
    window = disp[marks[warmup * c]:marks[-c]]                         # steps - 1 whole steps
    n = steps - 1
    own = ("k_adam", "k_grad_check", "k_ema", "amp_update_scale")
    by = {}
    for s, e, name in window:
        short = next((t for t in own if t in name), None)
        if short is None and "elementwise" in name:
            short = "torch_elementwise"
        if short:
            c = by.setdefault(short, [0, 0])
            c[0] += 1
            c[1] += e - s
    return {"kernel_ms_per_step": sum(e - s for s, e, _ in window) / n / 1e6, "launches_per_step": len(window) / n,
            "by_kernel_per_step": {k: {"launches": v[0] / n, "us": v[1] / n / 1e3} for k, v in sorted(by.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("a", "b", "c", "e", "swap"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--traced", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default=os.path.join(HERE, "_trace"))
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
    legs = ("a" if a.parent_tree else "") + "bce"
    me = os.path.abspath(__file__)
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--rays", str(a.rays), "--parent-tree", a.parent_tree]
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    for rep in range(1, a.repeats + 1):
        for leg in legs:            # alternating: a difference between legs is judged against the difference between a leg's own repeats
            label = f"{leg}_{rep}"
            subprocess.run([sys.executable, me, "--leg", leg, "--label", label, *common], check=True, timeout=300)
            out = os.path.join(a.out, label)
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            rc = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", label, "--",
                                 sys.executable, me, "--leg", leg, "--label", label, "--traced", *common], timeout=420).returncode
            if rc != 0:
                raise SystemExit(f"the traced run of leg {leg} ended with status {rc}: nothing more is started")
            print(json.dumps({"leg": leg, "label": label, "source": "rocprofv3 --kernel-trace --stats", "rc": rc, **trace_summary(out, a.warmup, a.steps)}), flush=True)
            for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
                os.remove(f)        # tens of MB per leg; the *_stats.csv files stay
    subprocess.run([sys.executable, me, "--leg", "swap", "--label", "swap", "--repeats", str(a.repeats)], check=True, timeout=300)


if __name__ == "__main__":
    main()
