#!/usr/bin/env python3
"""What the background model (bg_radius > 0) costs on an 800x800 frame: the fused launch (pnr_background_forward) by HIP events, the per-op chain
(sph_from_ray, [L,B,C] lookup + permute copy, SH, cat, two GEMMs, ReLU, sigmoid) in the same process, and the native lego / garden frames with and
without the background.  Reads nothing outside the repository; writes profiles/background/background_bench.json (or --out).

    python profiles/background_bench.py [--out FILE] [--only-launch N]     (--only-launch: N fused launches and nothing else, for a kernel trace)
    python profiles/background_bench.py --merge-trace STATS.csv            (adds that trace's k_background figures to the JSON)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palettenerf_amd import network, raymarching, scene  # noqa: E402
from palettenerf_amd.fused import background_fused  # noqa: E402

H = W = 800
HBM_TBS = 8.0       # the bandwidth figure the project's rooflines use


def model(cuda, bg_radius, bound=2, grid=None, density_scale=100.0):      # (bench.py's opaque field: density_scale 100)
    m = network.NeRFNetwork(bound=bound, cuda_ray=True, density_scale=density_scale, min_near=0.2, bg_radius=bg_radius)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid() if grid is None else grid).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field = "native", True
    return m


def timed(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background", "background_bench.json"))
    ap.add_argument("--only-launch", type=int, default=0)
    ap.add_argument("--merge-trace", help="a rocprofv3 kernel-stats CSV of an --only-launch run: its k_background rows go into the JSON (no GPU needed)")
    args = ap.parse_args()
    if args.merge_trace:
        import csv
        with open(args.out) as f:
            out = json.load(f)
        with open(args.merge_trace) as f:
            rows = [r for r in csv.DictReader(f) if "k_background" in r["Name"]]
        out["kernel_trace"] = [{"kernel": r["Name"], "calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                "max_us": float(r["MaxNs"]) / 1e3} for r in rows]
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        return
    cuda = torch.device("cuda:0")
    m = model(cuda, 4)
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    ro, rd = ro.to(cuda).view(-1, 3).contiguous(), rd.to(cuda).view(-1, 3).contiguous()
    N = ro.shape[0]
    bgf = background_fused(m)
    if args.only_launch:
        with torch.no_grad():
            for _ in range(args.only_launch):
                bgf.from_rays(ro, rd)
        torch.cuda.synchronize()
        return
    out = {"rays": N, "table_rows": int(m.encoder_bg.embeddings.shape[0])}
    with torch.no_grad():
        out["fused_launch"] = timed(lambda: bgf.from_rays(ro, rd))
        with torch.autocast("cuda", dtype=torch.float16):
            out["fused_launch_half_table"] = timed(lambda: bgf.from_rays(ro, rd))
        m.fused_field, m.march_mode = False, "compat"
        out["per_op_chain"] = timed(lambda: m.background(raymarching.sph_from_ray(ro, rd, m.bg_radius), rd))
        m.fused_field, m.march_mode = True, "native"
    # bytes the launch has to move: 6 floats in, 3 out per ray, and 16 gathers of 8 bytes per ray (the coarse levels hit in cache; the upper bound counts all)
    stream_bytes, gather_bytes = N * 9 * 4, N * 16 * 8
    t = out["fused_launch"]["median_ms"] * 1e-3
    out["bandwidth"] = {"stream_bytes": stream_bytes, "gather_bytes": gather_bytes, "achieved_TBs": (stream_bytes + gather_bytes) / t / 1e12,
                        "fraction_of_8TBs": (stream_bytes + gather_bytes) / t / 1e12 / HBM_TBS}
    frames = {}
    # lego: the brick scene from the blender-style pose, dt_gamma 0; garden: the garden-like scene from its orbit, cone stepping (dt_gamma 1/128)
    views = {"lego": (scene.lookat_pose(), scene.intrinsics_from_fov(H, W), None, 0.0),
             "garden": (scene.garden_orbit_pose(0), scene.garden_intrinsics(H, W), scene.garden_density_grid(), 1.0 / 128)}
    for name, (pose, intr, grid, dt_gamma) in views.items():
        fro, frd = scene.get_rays(torch.from_numpy(pose)[None].float(), intr, H, W)
        fro, frd = fro.to(cuda), frd.to(cuda)
        for tag, radius in (("plain", 0), ("background", 4)):
            fm = model(cuda, 4, 2, grid)
            fm.bg_radius = radius
            with torch.no_grad():
                frames[f"{name}_{tag}"] = timed(lambda: fm.render(fro, frd, dt_gamma=dt_gamma, perturb=False, max_steps=1024, T_thresh=1e-4), warmup=5, reps=40)
        frames[f"{name}_added_ms"] = frames[f"{name}_background"]["median_ms"] - frames[f"{name}_plain"]["median_ms"]
    out["frames"] = frames
    out["claim_added_below_per_op_chain"] = all(v < out["per_op_chain"]["median_ms"] for k, v in frames.items() if k.endswith("_added_ms"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
