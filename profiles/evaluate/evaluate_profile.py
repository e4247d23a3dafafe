"""The two launches behind a frame of the evaluate / test loops next to the same work as torch ops on the device (profiles/evaluate/README.md).

    python3 profiles/evaluate/evaluate_profile.py            legs at 800 x 800, nb = 4 (alternated, each twice) + test_path against render_path
    rocprofv3 --kernel-trace --stats --output-format csv -- python3 profiles/evaluate/evaluate_profile.py --once     20 native launches each, for the tracer

The torch legs are the reference's expressions with `.cpu()` removed -- what exists without pnr_palette_sheets / pnr_frame_metrics: the byte
expressions of palette/utils.py:993-1038 and the meters of nerf/utils.py:220-330 / palette/utils.py:52-114 (SSIM as F.pad + F.conv2d in fp32)."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from palettenerf_amd import _lib, network, pipeline, raymarching, renderer, scene   # noqa: E402
from palettenerf_amd import evaluate as ev   # noqa: E402

H = W = 800
NB = 4


def frame_maps(cuda, seed=0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    ch = int(_lib.load().pnr_palette_aux_channels(NB, 0))
    aux = torch.rand(H * W, ch, generator=g, device=cuda)
    r = {"image": torch.rand(H * W, 3, generator=g, device=cuda), "depth": torch.rand(H * W, generator=g, device=cuda),
         "direct_rgb": aux[:, 0:3], "view_dep_rgb": aux[:, 3:6], "basis_acc": aux[:, 6:6 + NB], "basis_rgb": aux[:, 6 + NB:6 + 4 * NB],
         "unscaled_basis_rgb": aux[:, 6 + 4 * NB:6 + 7 * NB]}
    truth = torch.rand(H, W, 4, generator=g, device=cuda)
    palette = torch.rand(NB, 3, generator=g, device=cuda)
    return r, truth, palette


def u8(x):
    return (x.clamp(0, 1) * 255).to(torch.uint8)


def torch_sheets(r, palette):
    """palette/utils.py:993-1038 on the device"""
    out = {"rgb": u8(r["image"].reshape(H, W, 3)), "depth": (r["depth"].reshape(H, W) * 255).to(torch.uint8),
           "view_dep": u8(r["view_dep_rgb"].reshape(H, W, 3)), "direct": u8(r["direct_rgb"].reshape(H, W, 3))}
    out["basis_img"] = u8(torch.cat([r["basis_rgb"][:, i * 3:(i + 1) * 3].reshape(H, W, 3) for i in range(NB)], dim=1))
    out["unscaled_basis_img"] = u8(torch.cat([r["unscaled_basis_rgb"][:, i * 3:(i + 1) * 3].reshape(H, W, 3) for i in range(NB)], dim=1))
    out["basis_acc"] = u8(torch.cat([r["basis_acc"][:, i:i + 1].reshape(H, W) for i in range(NB)], dim=1))
    out["basis_color"] = u8(torch.cat([palette[i, None, None, :].repeat(100, 100, 1).clamp(0, 1) for i in range(NB)], dim=1))
    return out


_K = None


def torch_metrics(pred, truth, omega):
    """eval_step's ground truth and the four meters on the device in fp32 (tests/evaluate_reference.py's text)"""
    global _K
    if _K is None:
        x = torch.arange(11, dtype=torch.float32, device=pred.device) - 5
        g = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
        g = g / g.sum()
        _K = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    gt = truth[..., :3] * truth[..., 3:] + (1 - truth[..., 3:])
    mse = ((pred - gt) ** 2).mean()
    psnr = -10 * torch.log10(mse)
    p, t = pred.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None]
    filt = lambda z: F.conv2d(F.pad(z, (5, 5, 5, 5), mode="reflect"), _K, groups=3)
    mu1, mu2 = filt(p), filt(t)
    s1, s2, s12 = filt(p * p) - mu1 * mu1, filt(t * t) - mu2 * mu2, filt(p * t) - mu1 * mu2
    S = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4) + 1e-12)
    ssim = 1 - 2 * torch.clamp((1 - S) / 2, 0, 1).mean()
    sp = (omega.sum(-1, keepdim=True) / ((omega ** 2).sum(-1, keepdim=True) + 1e-6) - 1).mean()
    tv = 100 * (torch.mean((omega[:, :-1] - omega[:, 1:]) ** 2) + torch.mean((omega[:-1] - omega[1:]) ** 2))
    return torch.stack([mse, psnr, ssim, sp, tv])


def timed(fn, iters):
    """mean ms per call over `iters` calls between two device synchronisations (host clock)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def path_model(cuda):
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=100.0, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field = "native", True
    return m


def main():
    cuda = torch.device("cuda:0")
    r, truth, palette = frame_maps(cuda)
    pred, omega = r["image"].reshape(H, W, 3), r["basis_acc"].reshape(H, W, NB)
    ms = ev.MeterSet(NB, want=("psnr", "ssim", "sparsity", "tv", "mse"))
    native_sheets = lambda: ev.frame_sheets(r, H, W, NB, basis_color=palette)
    native_metrics = lambda: ms.update(pred, truth, omega)
    if "--once" in sys.argv:
        for _ in range(20):
            native_sheets()
            native_metrics()
        torch.cuda.synchronize()
        print(json.dumps({"traced_launches_each": 20}))
        return
    legs = {"sheets_native": native_sheets, "sheets_torch": lambda: torch_sheets(r, palette), "metrics_native": native_metrics,
            "metrics_torch": lambda: torch_metrics(pred, truth, omega)}
    out = {k: [] for k in legs}
    for _ in range(2):                                   # alternate the legs, each twice
        for k, fn in legs.items():
            out[k].append(timed(fn, 50))
    fp32 = torch_metrics(pred, truth, omega).double().cpu()
    t = torch.tensor(ms.totals()[1:6], dtype=torch.float64) / ms.totals()[0]
    out["metrics_native_minus_torch_fp32"] = (t - fp32).tolist()
    sh, th = native_sheets(), torch_sheets(r, palette)
    out["sheets_equal_torch"] = {k: bool(torch.equal(sh[k], th[k])) for k in th}
    out["bytes_per_frame_to_host"] = {"reference_fp32_maps": H * W * 4 * (3 + 1 + 3 + 3 * NB + NB) + NB * 3 * 4,
                                      "sheets_uint8": int(sum(v.numel() for k, v in sh.items() if k in ("rgb", "depth", "view_dep", "basis_img", "basis_acc", "basis_color")))}
    m = path_model(cuda)
    poses = np.stack([scene.lookat_pose(azimuth_deg=18.0 * i) for i in range(20)])
    intr = scene.intrinsics_from_fov(H, W)
    kw = dict(perturb=False, bg_color=1, max_steps=1024, T_thresh=1e-4)
    paths = {"render_path": lambda: pipeline.render_path(m, poses, intr, H, W, frames_in_flight=1, **kw),
             "test_path": lambda: ev.test_path(m, poses, intr, H, W, frames_in_flight=1, **kw)}
    for k in paths:
        out[k + "_ms_per_frame"] = []
    for rep in range(3):                                 # the first repetition warms up (allocations, first launches); alternated
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                out[k + "_ms_per_frame"].append((time.perf_counter() - t0) * 1e3 / len(poses))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
