#!/usr/bin/env python3
"""How much of a PaletteNeRF training step is batch formation, and what `trainset.TrainSet.batch` makes of it.

Workload: a configs[3]-shaped step -- 4 096 rays from 17 views of 1008 x 756, RGBA fp16 stack on the device, per-pixel random background,
32^3 weight guide with 5 bases, slab scene, dt_gamma 1/128, train_step's loss, the one-launch Adam.
Legs:   parent  the batch as the tree formed one before: rays.get_rays + the reference's torch expressions (tests/train_batch_reference.py)
        new     TrainSet.batch (index and background draws by torch, then one launch)
Both legs choose the view by an index that is already on the device, so the parent leg pays no read-back for it (the reference does).

    python profiles/train_batch/measure.py run --out DIR      two repeats per leg, alternating, every child under its own time limit; then one
                                                              `rocprofv3 --kernel-trace --stats` child per leg; writes DIR/README.md
    python profiles/train_batch/measure.py leg --leg new      one leg in this process, prints one JSON line

Under the tracer a leg brackets its two timed regions (whole steps; batch formation alone) with a launch no step makes (k_image_to_uint8):
launches and kernel time per step are counted between those markers."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
MARKER = "k_image_to_uint8"
RAYS, VIEWS, H, W, NB, S = 4096, 17, 756, 1008, 5, 32


def setup(dev):
    import numpy as np
    import torch
    from palettenerf_amd import network, optim, raymarching, renderer, scene, trainset
    torch.manual_seed(0)
    g = np.random.default_rng(0)
    hist = g.random((S, S, S, NB)).astype(np.float32)
    hist /= hist.sum(-1, keepdims=True)
    m = network.PaletteNetwork(renderer.default_opt(test=False, num_basis=NB), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m.initialize_palette(g.random((NB, 3)).tolist(), hist_weights=hist)
    m = m.to(dev).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(dev))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    poses = []
    for i in range(VIEWS):
        a = 2 * np.pi * i / VIEWS
        p = np.eye(4, dtype=np.float32)
        p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3 * np.cos(a), 0.3 * np.sin(a), 1.5]
        poses.append(p)
    images = torch.rand(VIEWS, H, W, 4, device=dev).half()
    ts = trainset.TrainSet(images, np.stack(poses), scene.intrinsics_from_fov(H, W, 0.9), H, W, RAYS, storage="fp16")
    opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    return m, ts, opt


def run_leg(leg, steps, warmup):
    import torch
    from palettenerf_amd import rays, trainset
    from tests import train_batch_reference as ref
    dev = torch.device("cuda:0")
    m, ts, opt = setup(dev)
    order = torch.arange(4096, device=dev) % VIEWS
    render = dict(dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4)
    lam = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_weight=0.05, lambda_palette=1e-3)

    def batch(i):
        vi = order[i:i + 1]
        if leg == "new":
            return ts.batch(vi, m)
        p = ref.parent_batch(ts.poses, ts.intrinsics, H, W, RAYS, ts.images, vi, hist_weights=m.hist_weights)
        return trainset.TrainBatch(p["rays_o"], p["rays_d"], p["gt_rgb"], p["bg_color"], p["gt_weights"], None, p["inds"], None, vi, H, W)

    def step(i):
        opt.zero_grad(set_to_none=True)
        _, _, loss, _ = trainset.train_step(m, batch(i), render, want_outputs=False, **lam)
        loss.backward()
        opt.step()

    def mark():
        rays.image_to_uint8(torch.zeros(4, device=dev))

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / max(1, n) * 1e3

    for i in range(warmup):
        step(i)
    timed(batch, warmup)
    mark()
    step_ms = timed(step, steps)
    mark()
    batch_ms = timed(batch, steps)
    mark()
    torch.cuda.synchronize()
    print(json.dumps({"leg": leg, "steps": steps, "step_ms": step_ms, "batch_ms": batch_ms}))


def trace_regions(path, steps):
    """Per step, between the markers of a traced leg: launches and kernel microseconds of (whole steps, batch formation alone), and the kernel names
    of one batch formation with their counts."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    if len(marks) != 3:
        raise RuntimeError(f"{path}: expected 3 marker launches, found {len(marks)}")
    out = []
    for a, b in zip(marks, marks[1:]):
        seg = rows[a + 1:b]
        out.append((len(seg) / steps, sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / 1e3 / steps))
    names = {}
    for r in rows[marks[1] + 1:marks[2]]:
        n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("at::native::", "")[:110]
        names[n] = names.get(n, 0) + 1
    return out[0], out[1], {k: v / steps for k, v in sorted(names.items(), key=lambda kv: -kv[1])}


def child(cmd, limit, log):
    """One GPU child under its own time limit; anything but a clean exit ends the measurement."""
    try:
        r = subprocess.run(cmd, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"time limit of {limit} s: {' '.join(cmd)}")
    open(log, "a").write(r.stdout)
    if r.returncode != 0:
        raise SystemExit(f"exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}")
    return r.stdout


def run(out, steps, warmup, trace_steps):
    os.makedirs(out, exist_ok=True)
    log = os.path.join(out, "children.log")
    me = [sys.executable, os.path.abspath(__file__), "leg"]
    wall = {"parent": [], "new": []}
    for leg in ("parent", "new", "parent", "new"):
        text = child(me + ["--leg", leg, "--steps", str(steps), "--warmup", str(warmup)], 240, log)
        wall[leg].append(json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1]))
    traces = {}
    for leg in ("parent", "new"):
        d = os.path.join(out, "trace_" + leg)
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", leg, "--"] + me
              + ["--leg", leg, "--steps", str(trace_steps), "--warmup", "5"], 300, log)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        traces[leg] = trace_regions(found[0], trace_steps)
    lines = ["# Batch formation of a PaletteNeRF training step: `rays.get_rays` + torch expressions against `TrainSet.batch`", "",
             f"Made by `profiles/train_batch/measure.py run` on one MI355X.  Workload: {RAYS} rays from {VIEWS} views of {W} x {H}, RGBA fp16 stack, per-pixel",
             f"random background, {S}^3 weight guide with {NB} bases, slab scene, `train_step` + backward + one-launch Adam.  Legs alternate in fresh processes",
             f"(parent, new, parent, new), {steps} timed steps after {warmup} warm-up steps each; both legs take the view index from the device.", "",
             "## Wall time (ms per step, host clock around a synchronised loop)", "", "| leg | run | whole step | batch formation alone |", "|---|---|---|---|"]
    for leg in ("parent", "new"):
        for i, r in enumerate(wall[leg]):
            lines.append(f"| {leg} | {i + 1} | {r['step_ms']:.3f} | {r['batch_ms']:.3f} |")
    lines += ["", f"## Launches and kernel time per step (`rocprofv3 --kernel-trace --stats`, a run of its own per leg, {trace_steps} steps)", "",
              "| leg | launches, whole step | kernel us, whole step | launches, batch formation | kernel us, batch formation |", "|---|---|---|---|---|"]
    for leg in ("parent", "new"):
        (sl, su), (bl, bu), _ = traces[leg]
        lines.append(f"| {leg} | {sl:.1f} | {su:.1f} | {bl:.1f} | {bu:.1f} |")
    for leg in ("parent", "new"):
        lines += ["", f"Kernels of one batch formation, {leg} leg (launches per step):", ""] + [f"* {v:.2f} x `{k}`" for k, v in traces[leg][2].items()]
    p, n = [statistics.mean(r["step_ms"] for r in wall[k]) for k in ("parent", "new")]
    spread = max(r["step_ms"] for r in wall["parent"]) - min(r["step_ms"] for r in wall["parent"])
    lines += ["", f"Whole step, mean of the two runs: parent {p:.3f} ms, new {n:.3f} ms (difference {p - n:+.3f} ms; the parent leg's two runs differ by {spread:.3f} ms).", ""]
    open(os.path.join(out, "README.md"), "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "leg"])
    ap.add_argument("--leg", choices=["parent", "new"], default="new")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    a = ap.parse_args()
    if a.mode == "leg":
        run_leg(a.leg, a.steps, a.warmup)
    else:
        run(a.out, a.steps, a.warmup, a.trace_steps)
