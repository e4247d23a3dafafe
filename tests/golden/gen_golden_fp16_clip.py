#!/usr/bin/env python3
"""Generate frame_palette_fp16_clip_{a,b}.npz: the reference's PaletteNeRF inference frame with the clip head (--pred_clip --clip_dim 16) in its
-O mode (half hash tables) and beside it the same frame with fp32 tables.  Run in the BUILD container only (it reads the reference through
gen_golden.import_reference(); the fixtures it writes are data).

  * The reference's own PaletteNetwork.run_cuda, the CPU oracle injected as the kernel layer (gen_golden.import_reference explains).
  * -O: torch.is_autocast_enabled is forced to True (as gen_golden.gen_grid_autocast does) -- the flag is all gridencoder/grid.py:38-39 looks at:
    the kernel then gets `embeddings.to(torch.half)` and returns half features.  The reference's MLPs cannot take half inputs on the CPU, so the
    output of each of the three encoder instances (encoder, encoder_palette, encoder_clip) is upcast with .float(): half lookups, then an fp32
    field -- the project's -O frame.
  * Every frame runs in a child process of its own: after one forced-half frame a later fp32 frame in the same process still got half features.
  * Table scale: with the tables as scene.seed_field_ makes them the half and fp32 frames differ by ~1e-6, below any colour tolerance, and a
    golden could not tell fp32 lookups from half ones.  All three tables are multiplied by SCALE (a power of two: exact) after seeding; the
    tests do the same on the device.
  * Each case asserts that the reference's half and fp32 frames differ on `image` and `clip_feat` by at least 10x the tolerance the GPU test
    uses (TOL; tests/test_gpu_fp16_clip.py explains how it was measured).
Weights are not stored: the fixtures carry the seed and the scale."""
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402
from gen_golden import frame_inputs, setup_model  # noqa: E402
from palettenerf_amd import scene  # noqa: E402

SCALE = 64.0
TOL = 1e-4          # the GPU test's tolerance on image and clip_feat (tests/test_gpu_fp16_clip.py: max(1e-4, 4 x measured))
CASES = [
    # name, H, W, dt_gamma, density_scale, seed
    ("a", 40, 40, 0.0, 1.0, 100),
    ("b", 36, 28, 1.0 / 128, 0.02, 101),
]
KEYS = ["image", "depth", "depth_origin", "weights_sum", "clip_feat", "direct_rgb", "view_dep_rgb", "basis_rgb", "unscaled_basis_rgb", "basis_acc"]


def render(name, half, out_path):
    """One frame of the reference (child process)."""
    _ref_nerf, ref_pal, _ref_pal_r = gen_golden.import_reference()
    _, H, W, dt_gamma, dscale, seed = [c for c in CASES if c[0] == name][0]
    ro, rd = frame_inputs(H, W)
    opt = types.SimpleNamespace(num_basis=4, clip_dim=16, pred_clip=True, use_initialization_from_rgbxy=False, test=True,
                                color_space="srgb", smooth_sigma_xyz=0.005, smooth_sigma_color=0.2, smooth_sigma_clip=0.0)
    p = ref_pal.PaletteNetwork(opt, bound=2, cuda_ray=True, density_scale=dscale, min_near=0.2)
    scene.seed_field_(p, seed)
    with torch.no_grad():
        for enc in (p.encoder, p.encoder_palette, p.encoder_clip):
            enc.embeddings.mul_(SCALE)
    setup_model(p, scene.brick_density_grid())
    p.eval()
    for enc in (p.encoder, p.encoder_palette, p.encoder_clip):   # half lookups -> fp32 field (instance attribute: nn.Module.__call__ finds it)
        enc.forward = (lambda f: lambda *a, **k: f(*a, **k).float())(enc.forward)
    real = torch.is_autocast_enabled
    if half:
        torch.is_autocast_enabled = lambda *a, **k: True
    try:
        with torch.no_grad():
            r = p.run_cuda(ro, rd, dt_gamma=dt_gamma, perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=False)
    finally:
        torch.is_autocast_enabled = real
    np.savez(out_path, **{k: r[k].float().numpy() for k in KEYS})


def main():
    for name, H, W, dt_gamma, dscale, seed in CASES:
        maps = {}
        with tempfile.TemporaryDirectory() as tmp:
            for half in (True, False):
                path = os.path.join(tmp, f"{name}_{int(half)}.npz")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(int(half)), path], check=True)
                with np.load(path) as z:
                    maps[half] = {k: z[k] for k in KEYS}
        gap = {k: float(np.abs(maps[True][k] - maps[False][k]).max()) for k in KEYS}
        print(name, "half vs fp32:", " ".join(f"{k} {v:.3g}" for k, v in gap.items()),
              "| image range", float(maps[True]["image"].min()), float(maps[True]["image"].max()))
        for k in ("image", "clip_feat"):
            assert gap[k] >= 10 * TOL, (name, k, gap[k])
        np.savez_compressed(os.path.join(HERE, f"frame_palette_fp16_clip_{name}.npz"), H=H, W=W, dt_gamma=dt_gamma, density_scale=dscale, seed=seed,
                            pred_clip=True, scale=SCALE, **{f"half_{k}": v for k, v in maps[True].items()},
                            **{f"fp32_{k}": v for k, v in maps[False].items()})


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        render(sys.argv[2], bool(int(sys.argv[3])), sys.argv[4])
    else:
        main()
