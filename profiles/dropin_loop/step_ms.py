"""What a caller who keeps the reference's run_cuda pays per 800x800 inference frame, on bench.py's lego (NeRF) and lego_palette workloads (its model
builder, ray bank and timed loop, imported -- bench.py itself is not edited).  One leg per process, one JSON line on stdout:

    python profiles/dropin_loop/step_ms.py --leg a     # dropin.install() only: the per-op loop an unchanged run_cuda issues, torch nn.Linear MLPs
    python profiles/dropin_loop/step_ms.py --leg b     # + dropin.fuse_field(model)
    python profiles/dropin_loop/step_ms.py --leg c     # + dropin.fuse_loop(model): the same caller, its run_cuda bound to the native frame call
    python profiles/dropin_loop/step_ms.py --leg d     # this package's class with march_mode = "native": render(), one call per frame (the target)
    ... --workload lego_palette                        # PaletteNeRF (default: lego)

The caller of legs a-c is the one bench.dropin_leg uses: this package's mirror class left in its default `compat` mode, which issues exactly what
an unchanged run_cuda issues.  Legs c and d get the same initial ray order (--ray-order, bench.py's default tile8) and time the same loop
(bench.timed_frames: wall ms per frame over --steps frames of the orbit after --warmup, one synchronize at the end).  Legs that are compared run
in one session on one machine, alternating, three processes each; the spread of leg d's repeats is the yardstick for c - d
(profiles/dropin_loop/README.md)."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["a", "b", "c", "d"], required=True)
    ap.add_argument("--workload", choices=["lego", "lego_palette"], default="lego")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ray-order", default="tile8")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)

    import torch
    import bench
    from palettenerf_amd import dist as pdist, dropin
    from palettenerf_amd.fused import tile_ray_order
    if not torch.cuda.is_available():
        raise SystemExit("step_ms.py measures on a GPU; none is visible")
    device = torch.device("cuda:0")
    args = bench.parse(["--workload", a.workload, "--no-cpu-baseline", "--warmup", str(a.warmup), "--ray-order", a.ray_order])
    args.mode = "native" if a.leg == "d" else "compat"
    kind = args.wl["model"]
    H, W = args.wl["H"], args.wl["W"]
    idx, _ = pdist.shard_indices(H, W, 0, 1)
    bank = bench.RayBank(args, 1, idx, device)
    dropin.install()
    m = bench.build_model(args, device, kind)
    if a.leg in ("b", "c"):
        dropin.fuse_field(m, args.field_precision)
    if a.leg == "c":
        dropin.fuse_loop(m, args.field_precision)
    if a.leg in ("c", "d") and a.ray_order != "rowmajor":
        m._fused.ray_order = tile_ray_order(idx, W, {"tile8": 8, "tile4": 4, "tile16": 16, "morton": 0}[a.ray_order]).to(device)
    kw = dict(perturb=False, dt_gamma=args.wl["dt_gamma"], max_steps=1024, T_thresh=1e-4)
    if kind == "palette":
        kw["gui_mode"] = False
    bench.timed_frames(m, bank, kw, a.warmup, False)
    ms, rendered = bench.timed_frames(m, bank, kw, a.steps, False, first_step=a.warmup)
    ro, rd = bank.get(a.warmup)
    with torch.no_grad():
        r = m.render(ro, rd, **kw)
    print(json.dumps({"label": a.label, "leg": a.leg, "workload": a.workload, "res": [H, W], "ms_per_frame": ms, "rendered_per_frame": rendered, "steps": a.steps,
                      "warmup": a.warmup, "march_mode": m.march_mode, "native_frame": "iterations" in r, "run_cuda_bound": "run_cuda" in m.__dict__,
                      "forward_bound": "forward" in m.__dict__, "ray_order": a.ray_order if a.leg in ("c", "d") else None,
                      "image_mean": float(torch.nan_to_num(r["image"]).mean())}))


if __name__ == "__main__":
    main()
