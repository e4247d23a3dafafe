#!/usr/bin/env python3
"""Viewer frames of a still camera, 800x800, bench.py's lego (NeRF) and lego_palette (PaletteNeRF) models, gui_mode=True, fp32 and --fp16:

  jittered  pipeline.viewer_frame(spp=2): the native frame loop with the first-sample jitter + pnr_present_frame
  per_op    the same jittered frame the way the parent commit rendered it: the per-op loop (march_mode 'device'; for PaletteNeRF with the fused
            field in fp32 and the reference-style ops under autocast, which is where perturb sent it)
  plain     model.render(perturb=False) on the native loop: the unjittered native frame

and pnr_present_frame against the torch expressions it replaces (median wall time per call; kernel counts come from a rocprofv3 --kernel-trace
--stats run of this script with --present-only).  python profiles/viewer_bench.py OUT_DIR [--present-only] [--steps K]; writes OUT_DIR/viewer_bench.json.

--plain-only [--package-root DIR]: the `plain` row alone, with the palettenerf_amd package (and its built library) of another checkout when DIR is
given -- the parent commit's unjittered native frame on the same GPU, in a process of its own; writes OUT_DIR/plain_bench.json."""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if "--package-root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, ROOT)

from palettenerf_amd import network, pipeline, raymarching, renderer, scene  # noqa: E402
from palettenerf_amd import rays as prays  # noqa: E402
from palettenerf_amd.fused import NeRFFieldFused, PaletteFieldFused, tile_ray_order  # noqa: E402

H = W = 800
KW = dict(dt_gamma=0.0, max_steps=1024, T_thresh=1e-4)


def model_of(kind, dev):
    if kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    else:
        m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(dev).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(dev))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field = "native", True
    m._fused = (NeRFFieldFused if kind == "nerf" else PaletteFieldFused)(m)
    m._fused.ray_order = tile_ray_order(torch.arange(H * W), W, 8).to(dev)
    return m


def median_ms(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    out_dir = sys.argv[1]
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 30
    present_only = "--present-only" in sys.argv
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda:0")
    pose = scene.lookat_pose(azimuth_deg=45.0)
    intr = scene.intrinsics_from_fov(H, W)
    ro, rd = prays.rays_from_indices(torch.from_numpy(pose).float().reshape(1, 4, 4).to(dev), intr, H, W, None)
    res = {}
    if "--plain-only" in sys.argv:
        for kind in ("palette", "nerf"):
            m = model_of(kind, dev)
            gui = {"gui_mode": True} if kind == "palette" else {}
            for fp16 in (False, True):
                def plain():
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
                        return m.render(ro, rd, perturb=False, **gui, **KW)
                res[f"{kind} {'fp16' if fp16 else 'fp32'} plain_native_ms"] = median_ms(plain, steps)
        res["package"] = os.path.dirname(os.path.abspath(network.__file__))
        for k, v in res.items():
            print(f"{k}: {v}")
        with open(os.path.join(out_dir, "plain_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    for kind in ("palette", "nerf"):
        pal = kind == "palette"
        m = model_of(kind, dev)
        gui = {"gui_mode": True} if pal else {}
        with torch.no_grad():
            r = m.render(ro, rd, perturb=False, **gui, **KW)
            for name, (rh, rw) in (("800", (H, W)), ("400->800", (H // 2, W // 2))):
                n = rh * rw
                sub = {k: v.reshape(1, H * W, -1)[:, :n].contiguous() for k, v in r.items() if torch.is_tensor(v) and v.numel() >= H * W}
                args = dict(rays_o=ro[:, :n].contiguous(), rays_d=rd[:, :n].contiguous(), depth_origin=sub["depth_origin"], clip_feat=sub["clip_feat"]) if pal else {}

                def hip():
                    return pipeline.present_frame(sub["image"], sub["depth"], rh, rw, H, W, **args)

                def tor():
                    up = (lambda t: t) if (rh, rw) == (H, W) else (lambda t: F.interpolate(t.permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1).contiguous())
                    o = [up(sub["image"].reshape(1, rh, rw, 3).clamp(0, 1)), up(sub["depth"].reshape(1, rh, rw, 1))]
                    if pal:
                        o.append(up((args["rays_o"] + args["rays_d"] * sub["depth_origin"].reshape(1, n, 1)).reshape(1, rh, rw, 3)))
                        o.append(up(sub["clip_feat"].reshape(1, rh, rw, -1)).contiguous())
                    return o

                res[f"{kind} present {name} hip_ms"] = median_ms(hip, steps)
                res[f"{kind} present {name} torch_ms"] = median_ms(tor, steps)
        if present_only:
            continue
        for fp16 in (False, True):
            tag = f"{kind} {'fp16' if fp16 else 'fp32'}"

            def ctx():
                return torch.autocast("cuda", dtype=torch.float16, enabled=fp16)

            def jittered():
                with ctx():
                    return pipeline.viewer_frame(m, pose, intr, W, H, spp=2, **KW)

            def plain():
                with torch.no_grad(), ctx():
                    return m.render(ro, rd, perturb=False, **gui, **KW)

            def per_op():
                with torch.no_grad(), ctx():
                    return m.render(ro, rd, perturb=2, **gui, **KW)

            m.march_mode, m.fused_field = "native", True
            res[f"{tag} plain_native_ms"] = median_ms(plain, steps)
            res[f"{tag} jittered_viewer_frame_ms"] = median_ms(jittered, steps)
            res[f"{tag} plain_native_again_ms"] = median_ms(plain, steps)
            m.march_mode, m.fused_field = "device", (pal and not fp16)
            res[f"{tag} jittered_per_op_ms"] = median_ms(per_op, max(5, steps // 3), warmup=2)
    for k, v in res.items():
        print(f"{k}: {v:.3f}")
    with open(os.path.join(out_dir, "viewer_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
