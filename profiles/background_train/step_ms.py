"""One training step of a model WITH a background (bg_radius > 0): the configs[3]-shaped step of bench.make_training_step -- 4 096 random rays
of the 17-camera rig over the slab scene, dt_gamma 1/128, optim.Adam -- for the NeRF or the PaletteNeRF model.  Runs --warmup + --steps steps and
prints one JSON line (wall ms per step over the timed steps).  Kernel time and launch counts come from running this file under
`rocprofv3 --kernel-trace --stats` in a run of its own (profiles/background_train/README.md); a run with --steps 0 --warmup 0 gives the set-up's
share of those totals.

    python profiles/background_train/step_ms.py --kind nerf                    # this commit: fused background each way, train_loss
    python profiles/background_train/step_ms.py --kind nerf --per-op           # fused_train_background = False (train_loss still takes the [N,3] gradient)
    python profiles/background_train/step_ms.py --kind nerf --torch-loss --tree ../parent
                                                                               # the parent commit: its train_loss refuses a trainable background,
                                                                               # so the loss is the torch formulation on the result dict
    python profiles/background_train/step_ms.py --kind nerf --bg-radius 0      # a model without a background: the step this commit must not change
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["nerf", "palette"], default="nerf")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--bg-radius", type=float, default=4.0)
    ap.add_argument("--per-op", action="store_true")
    ap.add_argument("--torch-loss", action="store_true")
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    import numpy as np
    import torch
    import palettenerf_amd
    from palettenerf_amd import fused, network, optim, raymarching, renderer, scene
    from palettenerf_amd.train_loss import train_loss
    if not torch.cuda.is_available():
        raise SystemExit("step_ms.py measures on a GPU; none is visible")
    device = torch.device("cuda:0")
    if a.kind == "palette":
        m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True, min_near=0.02, bg_radius=a.bg_radius)
    else:
        m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.02, bg_radius=a.bg_radius)
    scene.seed_field_(m, 0)
    m = m.to(device).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(device))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.fused_field = True                            # the model asks for fused kernels (the condition of the background launches)
    m.fused_train_background = not a.per_op         # (a checkout without the training launches ignores it)
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
    lam = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_palette=1e-3)     # main_palette.py:83-89
    origin = (m.basis_color.detach() + 0.02).clone() if a.kind == "palette" else None

    def step(i):
        inds = inds_all[i % 64]
        ro, rd = ro_all[i % 17, inds][None], rd_all[i % 17, inds][None]
        opt.zero_grad(set_to_none=True)
        r = m.run_cuda(ro, rd, dt_gamma=1 / 128, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=1e-4)
        if not a.torch_loss:
            if a.kind == "palette":
                loss, _ = train_loss(r, target, basis_color=m.basis_color, basis_color_origin=origin, **lam)
            else:
                loss, _ = train_loss(r, target)
        else:           # bench.make_training_step's torch_loss branch: the trainer's loss on the lazy dict entries
            loss = ((r["image"] - target) ** 2).mean(-1)
            if a.kind == "palette":
                loss = loss + lam["lambda_sparsity"] * r["omega_sparsity"].mean() + lam["lambda_offsets"] * r["offsets_norm"].mean()
                loss = loss + lam["lambda_view_dep"] * r["view_dep_norm"].mean()
                loss = loss + lam["lambda_palette"] * ((m.basis_color - origin) ** 2).sum(dim=-1).mean()
                loss = loss + ((r["direct_rgb"] - target) ** 2).mean()
            loss = loss.mean()
        loss.backward()
        opt.step()
        return loss

    loss = None
    for i in range(a.warmup):
        loss = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss = step(a.warmup + i)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / max(a.steps, 1) * 1e3
    rec = {"label": a.label, "package": os.path.dirname(os.path.abspath(palettenerf_amd.__file__)), "kind": a.kind, "bg_radius": a.bg_radius,
           "fused_train_background": bool(not a.per_op and a.bg_radius > 0 and hasattr(fused, "background_train_fused")), "torch_loss": a.torch_loss,
           "steps": a.steps, "warmup": a.warmup, "rays_per_step": a.rays, "wall_ms_per_step": wall if a.steps else None}
    if loss is not None:
        rec["samples_per_step"] = int(m.step_counter[(m.local_step - 1) % 16, 0])
        rec["loss_last"] = float(loss)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
