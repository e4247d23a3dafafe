"""Figures of the palette extraction's front end (profiles/extract/README.md), one MI355X.

  python3 profiles/extract/measure.py [--views N] [--out FILE]     wall times of both legs, alternating, profiler off: JSON lines
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o extract -- python3 profiles/extract/measure.py --once
                                                                     one extract_centers and one extract_centers_per_op under the tracer

Model: bench.py's configs[2] shape -- a PaletteNetwork (4 bases) on the brick scene S0, scene.seed_field_(..., 0), bound 2, density_scale 100 --
at 800 x 800 over a handful of synthetic views (a smooth colour field plus noise as a uint8 TrainSet).  The baseline is the per-op leg at the same commit; nothing of the kind existed before."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from palettenerf_amd import extract, network, raymarching, renderer, scene, trainset  # noqa: E402

H = W = 800
KW = dict(max_steps=1024, T_thresh=1e-4)


def setup(cuda, views):
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field = "native", True
    intr = scene.intrinsics_from_fov(H, W)
    poses = np.stack([scene.lookat_pose(azimuth_deg=360.0 * i / views) for i in range(views)])
    # a smooth colour field plus noise: a few dozen heavy coarse bins, as a capture has (uniform noise alone gives no bin above tau)
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    img = np.empty((views, H, W, 4), dtype=np.uint8)
    for v in range(views):
        base = np.stack([xx, yy, 0.5 + 0.5 * np.sin(6.0 * (xx + yy) + v)], axis=-1)
        img[v, ..., :3] = np.clip((base + rng.normal(0, 0.03, size=base.shape)) * 255, 0, 255).astype(np.uint8)
        img[v, ..., 3] = 255
    ts = trainset.TrainSet(img, poses, intr, H, W, num_rays=4096, storage="uint8", device=cuda)
    return m, poses, intr, ts


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    cuda = torch.device("cuda:0")
    views = int(sys.argv[sys.argv.index("--views") + 1]) if "--views" in sys.argv else 5
    m, poses, intr, ts = setup(cuda, views)
    fused = lambda: extract.extract_centers(m, poses, intr, H, W, ts, **KW)            # noqa: E731
    per_op = lambda: extract.extract_centers_per_op(m, poses, intr, H, W, ts, **KW)   # noqa: E731
    if "--once" in sys.argv:
        a, b = fused(), per_op()
        torch.cuda.synchronize()
        print(json.dumps({"K": a["info"]["K"], "P": a["info"]["P"], "total": a["total"], "per_op_total": b["total"]}))
        return
    lines = []
    a, b = fused(), per_op()                                                           # warm-up: first use of every kernel
    rec = {"views": views, "H": H, "W": W, "valid": a["total"], "K": a["info"]["K"], "P": a["info"]["P"], "iterations": a["info"]["iterations"],
           "stop": a["info"]["stop"], "emptied": a["info"]["emptied"], "per_op_iterations": b["info"]["iterations"],
           "tables_equal": bool(np.array_equal(a["hist_fine"], b["hist_fine"]) and np.array_equal(a["hist_coarse"], b["hist_coarse"])),
           "table_l1": float(np.abs(a["hist_fine"] - b["hist_fine"]).sum() * a["total"]),
           "centres_max_diff_vs_per_op": float(np.abs(a["centers"] - b["centers"]).max()) if a["centers"].shape == b["centers"].shape else None}
    # the per-op leg with the float64 host k-means (the device's own arithmetic, another summation order), and scikit-learn's float32 run matched
    # centre by centre (its order and, on lattice points, its tie decisions are its own)
    c = extract.extract_centers_per_op(m, poses, intr, H, W, ts, kmeans="host", **KW)
    rec["per_op_host_kmeans_iterations"] = c["info"]["iterations"]
    rec["centres_max_diff_vs_per_op_host_kmeans"] = float(np.abs(a["centers"] - c["centers"]).max()) if a["centers"].shape == c["centers"].shape else None
    if a["centers"].shape == b["centers"].shape:
        d = np.sqrt(((a["centers"][:, None, :] - b["centers"][None, :, :]) ** 2).sum(-1))
        rec["centres_nearest_match_vs_sklearn_max"] = float(d.min(axis=1).max())
        rec["centres_nearest_match_vs_sklearn_median"] = float(np.median(d.min(axis=1)))
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    walls = {"fused_ms": [], "per_op_ms": []}
    for _ in range(5):                                                                  # legs alternating
        walls["fused_ms"].append(timed(fused)[1])
        walls["per_op_ms"].append(timed(per_op)[1])
    lines.append(walls)
    print(json.dumps(walls), flush=True)
    # the stages of the fused leg one by one: the frames alone, frames + accumulate, the k-means launch with its read-back
    from palettenerf_amd import pipeline
    from palettenerf_amd import rays as prays
    dposes = torch.from_numpy(poses).to(cuda)
    kw = dict(KW, bg_color=None, perturb=False, gui_mode=True)
    frames = lambda: pipeline.render_queue(m, lambda i: prays.rays_from_indices(dposes[i:i + 1], intr, H, W, None), views, consume=lambda i, r: None, **kw)   # noqa: E731
    stages = {"frames_only_ms": [], "frames_and_accumulate_ms": [], "kmeans_with_read_back_ms": [], "accumulate_event_ms": []}
    hist = extract.radiance_histograms(m, poses, intr, H, W, ts, **KW)
    ws = torch.rand(H * W, device=cuda)
    for _ in range(5):
        stages["frames_only_ms"].append(timed(frames)[1])
        stages["frames_and_accumulate_ms"].append(timed(lambda: extract.radiance_histograms(m, poses, intr, H, W, ts, **KW))[1])
        stages["kmeans_with_read_back_ms"].append(timed(lambda: extract.kmeans_centers(hist))[1])
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        scratch = extract.RadianceHistogram(cuda)
        e0.record()
        scratch.update(ws, ts.images[0])
        e1.record()
        torch.cuda.synchronize()
        stages["accumulate_event_ms"].append(e0.elapsed_time(e1))
    lines.append(stages)
    print(json.dumps(stages), flush=True)
    host = {"read_back_bytes_kmeans": (4 * 128 + 4) * 8, "read_back_bytes_tables": (512 + 32768 + 1) * 8,
            "per_op_read_back_bytes": int(a["total"]) * 3 * 4, "launches_per_view_accumulate": 1}
    lines.append(host)
    print(json.dumps(host), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
