"""Figures of profiles/distortion/README.md, measured on a GPU; prints JSON lines.

    python profiles/distortion/measure.py tolerance     # E of the per-op fp32 formulation and the kernel's own error, on the test batch
    python profiles/distortion/measure.py time          # the configs[3]-shaped batch: the operator and the padded dense torch formulation

`tolerance`: tests/distortion_reference.py's main batch; errors are max abs error over max abs value against float64, for dist and for
grad_sigmas (random grad_dist), of dr.per_op_fp32 on the device (E) and of raymarching.distortion_loss.
`time`: one training-mode run_cuda of bench.make_training_step("nerf", 4096 rays)'s model gives the batch (sigmas, deltas, rays); then
--reps forward + backward pairs of the operator, and as many of the padded dense formulation with its peak memory, both timed with events.
Kernel times come from running this mode under `rocprofv3 --kernel-trace --stats` (k_distortion_fwd / k_distortion_bwd in kernel_stats.csv)."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)


def rel(got, want):
    import numpy as np
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def tolerance(device):
    import torch
    from palettenerf_amd import raymarching
    from tests import distortion_reference as dr
    b, t = dr.batch("main"), dr.truth("main")
    dl, rays, g = (torch.from_numpy(b[k]).to(device) for k in ("dl", "rays", "gdist"))
    rec = {"mode": "tolerance", "rays": b["N"], "samples": b["M"], "max_dist": float(t["dist"].max()),
           "max_grad_sigmas": float(abs(t["grad_sigmas"]).max()), "closest_T_to_thresh": dr.check_batch(b)}
    for name, fn in (("per_op_fp32", dr.per_op_fp32), ("kernel", raymarching.distortion_loss)):
        s = torch.from_numpy(b["sig"]).to(device).requires_grad_(True)
        d = fn(s, dl, rays, dr.T_THRESH)
        (d * g).sum().backward()
        rec[name] = {"dist": rel(d.detach().cpu().numpy(), t["dist"]), "grad_sigmas": rel(s.grad.cpu().numpy(), t["grad_sigmas"])}
    print(json.dumps(rec))


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def time_(device, n_rays, reps):
    import torch
    import bench
    from palettenerf_amd import raymarching
    from tests import distortion_reference as dr
    m, step = bench.make_training_step("nerf", n_rays, device)
    seen, op = [], raymarching.distortion_loss
    raymarching.distortion_loss = lambda *a: (seen.append(a), op(*a))[1]
    step(0)                                              # (the bench's step: warms the model up; it does not ask for the map)
    torch.manual_seed(0)
    ro, rd = (t[None] for t in _rays(device, n_rays))
    m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=1e-4, distortion=True)
    raymarching.distortion_loss = op
    sigmas, deltas, rays, thresh = seen[0]
    sigmas, g = sigmas.detach(), torch.rand(rays.shape[0], device=device)
    M, N, longest = sigmas.shape[0], rays.shape[0], int(rays[:, 2].max())

    def run(fn):
        s = sigmas.clone().requires_grad_(True)
        (fn(s, deltas, rays, thresh) * g).sum().backward()
        return s.grad

    us_op = timed(lambda: run(op), reps)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    us_dense = timed(lambda: run(dr.per_op_fp32), reps)
    peak = torch.cuda.max_memory_allocated() - base
    ga, gb = run(op), run(dr.per_op_fp32)
    print(json.dumps({"mode": "time", "rays": N, "samples": M, "longest_ray": longest, "reps": reps, "operator_fwd_bwd_us_events": us_op,
                      "dense_fwd_bwd_us_events": us_dense, "dense_peak_bytes": int(peak), "dense_matrix_elements": N * longest,
                      "floor_fwd_us_12B_8TBs": M * 12 / 8e12 * 1e6, "floor_bwd_us_16B_8TBs": M * 16 / 8e12 * 1e6,
                      "grad_rel_diff_operator_vs_dense": float((ga - gb).abs().max() / gb.abs().max())}))


def _rays(device, n_rays):
    import numpy as np
    import torch
    from palettenerf_amd import scene
    H, W = 756, 1008
    p = np.eye(4, dtype=np.float32)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]      # camera 0 of the bench's rig
    ro, rd = scene.get_rays(torch.from_numpy(p)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    inds = torch.randint(0, H * W, [n_rays], generator=torch.Generator().manual_seed(0))
    return ro[0, inds].to(device), rd[0, inds].to(device)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["tolerance", "time"])
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    tolerance(dev) if a.mode == "tolerance" else time_(dev, a.rays, a.reps)
