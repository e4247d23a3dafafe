"""One NeRF-stage training step with the rgb_norm regulariser on (nerf/utils.py:527-536: rays_gt given to render, lambda_sparse = 0.05): the
configs[3]-shaped step of bench.make_training_step("nerf", ...) -- 4 096 rays, slab scene, dt_gamma 1/128, optim.Adam, the fused loss -- with
`rays_gt=target`.  Runs --warmup + --steps steps and prints one JSON line (wall ms per step over the timed steps, samples per step).  Kernel time
and launch counts come from running this file under `rocprofv3 --kernel-trace --stats` (profiles/sparse/README.md); a run with --steps 0
--warmup 0 gives the set-up's share of those totals.

    python profiles/sparse/step_ms.py                      # the fused composite (pnr_composite_rays_train_norm_*)
    python profiles/sparse/step_ms.py --per-op             # fused_train_norm = False: the branch as the reference writes it
    python profiles/sparse/step_ms.py --no-gt              # rays_gt = None: the step bench.py times
    python profiles/sparse/step_ms.py --tree ../parent     # the package of another (built) checkout, e.g. the parent commit

A checkout whose train_loss has no lambda_sparse adds the term as its docstring says the caller should: loss + lambda_sparse * rgb_norm.mean()."""
import argparse
import inspect
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--lambda-sparse", type=float, default=0.05)      # main_nerf.py:67
    ap.add_argument("--no-gt", action="store_true")
    ap.add_argument("--per-op", action="store_true")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    import numpy as np
    import torch
    import palettenerf_amd
    from palettenerf_amd import network, optim, raymarching, scene
    from palettenerf_amd.train_loss import train_loss
    if not torch.cuda.is_available():
        raise SystemExit("step_ms.py measures on a GPU; none is visible")
    device = torch.device("cuda:0")
    m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m = m.to(device).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(device))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.fused_train_norm = not a.per_op          # (a checkout without the fused composite ignores it)
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
    in_loss = "lambda_sparse" in inspect.signature(train_loss).parameters
    lam = 0.0 if a.no_gt else a.lambda_sparse

    def step(i):
        inds = inds_all[i % 64]
        ro, rd = ro_all[i % 17, inds][None], rd_all[i % 17, inds][None]
        opt.zero_grad(set_to_none=True)
        r = m.run_cuda(ro, rd, rays_gt=None if a.no_gt else target, dt_gamma=1 / 128, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
        if in_loss:
            loss, _ = train_loss(r, target, lambda_sparse=lam)
        else:
            loss, _ = train_loss(r, target)
            if lam:
                loss = loss + lam * r["rgb_norm"].mean()
        loss.backward()
        opt.step()
        return loss, r

    loss = r = None
    for i in range(a.warmup):
        loss, r = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss, r = step(a.warmup + i)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / max(a.steps, 1) * 1e3
    rec = {"label": a.label, "package": os.path.dirname(os.path.abspath(palettenerf_amd.__file__)), "rays_gt": not a.no_gt, "lambda_sparse": lam,
           "fused_train_norm": bool(not a.per_op and not a.no_gt and hasattr(raymarching, "composite_rays_train_norm")), "sparse_term_in_train_loss": in_loss,
           "steps": a.steps, "warmup": a.warmup, "rays_per_step": a.rays, "wall_ms_per_step": wall if a.steps else None}
    if r is not None:
        rec["samples_per_step"] = int(m.step_counter[(m.local_step - 1) % 16, 0])
        rec["loss_last"] = float(loss)
        rec["rgb_norm_mean_last"] = float(r["rgb_norm"].mean())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
