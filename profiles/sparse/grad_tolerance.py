#!/usr/bin/env python3
"""Where the gradient tolerance of tests/test_gpu_train_norm.py::test_model_step_fused_against_the_per_op_branch comes from: that test's 256-ray
NeRF step (rays_gt given, lambda_sparse = 0.05, binned table gradient) run through the per-op branch (fused_train_norm = False) and through the
fused composite, each against a float64 evaluation of the same step -- the samples the fp32 march produced, then hash grid, SH, both MLPs,
compositing with the reference's stop rule, the regulariser and the loss in float64 torch on the CPU.  Figure per parameter, as
profiles/grad_tolerance.py measures: max |g - g64| / max |g64|.  The test allows, per parameter, 4 x the per-op branch's figure."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F

import test_gpu_train_norm as T
from oracle.torch_encoders import TorchGridEncoder, TorchSHEncoder
from palettenerf_amd import gridencoder, renderer

cuda = torch.device("cuda:0")
gridencoder.BINNED_MIN_ROWS = 1
m = T.make_model(cuda)
seen = {}
march = renderer.raymarching.march_rays_train
renderer.raymarching.march_rays_train = lambda *a, **k: (lambda out: (seen.update(out=out), out)[1])(march(*a, **k))
try:
    per_op = T.train_step(m, False)
    xyzs, dirs, deltas, rays = [t.detach().cpu() for t in seen["out"]]
    fused = T.train_step(m, True)
    assert torch.equal(seen["out"][0].cpu(), xyzs)      # one seed, one perturbation
finally:
    renderer.raymarching.march_rays_train = march

# ---- the same step in float64
f64 = torch.float64
e = m.encoder
enc = TorchGridEncoder(num_levels=e.num_levels, level_dim=e.level_dim, per_level_scale=e.per_level_scale, base_resolution=e.base_resolution,
                       log2_hashmap_size=e.log2_hashmap_size)
assert torch.equal(enc.offsets, e.offsets.cpu())
enc.embeddings = torch.nn.Parameter(e.embeddings.detach().cpu().to(f64))
W = {n: p.detach().cpu().to(f64).requires_grad_(True) for n, p in m.named_parameters() if n.endswith(".weight")}
h = enc(xyzs.to(f64), bound=m.bound)
h = F.relu(h @ W["sigma_net.0.weight"].T) @ W["sigma_net.1.weight"].T
sigma, geo = torch.exp(h[:, 0]) * m.density_scale, h[:, 1:]
c = torch.cat([TorchSHEncoder(degree=4)(dirs.to(f64)), geo], -1)
c = F.relu(c @ W["color_net.0.weight"].T)
c = F.relu(c @ W["color_net.1.weight"].T)
rgb = torch.sigmoid(c @ W["color_net.2.weight"].T)
_, _, gt = T.rays256()
gt = gt.view(-1, 3).cpu().to(f64)
idx, off, cnt = rays[:, 0].long(), rays[:, 1].long(), rays[:, 2].long()
L = int(cnt.max())
k = torch.arange(L)[None]
valid = k < cnt[:, None]
row = (off[:, None] + k).clamp(max=xyzs.shape[0] - 1)
alpha = (1 - torch.exp(-sigma[row] * deltas[:, 0].to(f64)[row])) * valid
T_before = torch.cumprod(torch.cat([torch.ones(len(cnt), 1, dtype=f64), 1 - alpha[:, :-1]], 1), 1)
live = valid & (T_before.detach() >= T.T_THRESH)          # stop after the sample that sees T < T_thresh (raymarching.cu:566-572)
w = alpha * T_before * live
image = (w[..., None] * rgb[row]).sum(1)
ws = w.sum(1)
norm = (w * ((gt[idx][:, None] - rgb[row]) ** 2).sum(-1)).sum(1)
image = image + (1 - ws)[:, None] * 1.0                     # bg_color = 1
loss = (((image - gt[idx]) ** 2).mean(-1) + T.LAMBDA_SPARSE * norm).mean()
loss.backward()
g64 = {"encoder.embeddings": enc.embeddings.grad, **{n: p.grad for n, p in W.items()}}

print(f"samples {xyzs.shape[0]}, rays {len(cnt)}; loss fp32 per-op {float(per_op['loss']):.9e} fused {float(fused['loss']):.9e} float64 {float(loss.detach()):.9e}")
worst = {"per-op": 0.0, "fused": 0.0}
for n in sorted(g64):
    scale = float(g64[n].abs().max())
    line = f"{n:24s} max |g64| {scale:.3e}"
    for name, run in (("per-op", per_op), ("fused", fused)):
        err = float((run["grads"][n].cpu().to(f64) - g64[n]).abs().max()) / scale
        worst[name] = max(worst[name], err)
        line += f"   {name} vs float64 {err:.3e}"
    line += f"   fused vs per-op {float((fused['grads'][n] - per_op['grads'][n]).abs().max()) / float(per_op['grads'][n].abs().max()):.3e}"
    print(line)
print(f"== largest figure: per-op branch vs float64 {worst['per-op']:.3e}; fused vs float64 {worst['fused']:.3e}  (the per-op column is MEASURED_GRAD_ERR_VS_FLOAT64)")
