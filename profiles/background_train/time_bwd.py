"""Event-timed background launches at N = 4 096, with and without the table gradient, on two sets of rays: directions all over the sphere, and the
forward-facing rig of step_ms.py (whose rays share few cells of the coarse levels).  Prints the median and the minimum of 25 timed calls per entry
point (pnr_background_backward is both of its launches).

    python profiles/background_train/time_bwd.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main():
    import numpy as np
    import torch
    from palettenerf_amd import _torch_glue, network, scene
    from palettenerf_amd.fused import background_fused
    if not torch.cuda.is_available():
        raise SystemExit("time_bwd.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    N = 4096
    m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.02, bg_radius=4)
    scene.seed_field_(m, 0)
    m = m.to(dev).train()
    m.fused_field = True
    g = torch.Generator().manual_seed(1)
    sphere = ((torch.rand(N, 3, generator=g) * 2 - 1) * 1.5, torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1))
    H, W = 756, 1008
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]
    ro, rd = scene.get_rays(torch.from_numpy(pose)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    inds = torch.randint(0, H * W, [N], generator=g)
    rig = (ro[0, inds], rd[0, inds])
    w = torch.rand(N, 3, generator=g).to(dev)
    names = ["pnr_background_train_forward", "pnr_background_backward"]
    for label, (o, d) in (("sphere", sphere), ("rig", rig), ("sphere", sphere), ("rig", rig)):
        o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
        for table in (True, False):
            m.encoder_bg.embeddings.requires_grad_(table)
            prof = _torch_glue.profile_kernels(names)
            for _ in range(30):
                m.zero_grad(set_to_none=True)
                (background_fused(m).train_from_rays(o, d) * w).sum().backward()
            torch.cuda.synchronize()
            _torch_glue.profile_kernels(None)
            for k in names:
                ts = sorted(a.elapsed_time(b) * 1e3 for a, b, _ in prof[k][5:])
                print(f"{label:6s} table_grad={table!s:5s} {k}: median {ts[len(ts) // 2]:.1f} us, min {ts[0]:.1f} us")


if __name__ == "__main__":
    main()
