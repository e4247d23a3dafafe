"""A float64 statement of the Stylizer fit (palette/gui.py:153-194 as pnr_stylizer_fit states it in include/pnr.h) for the stylize tests:
the loss by torch autograd, plain SGD with momentum, the learning rates of stylize.lr_table narrowed to fp32 as every fp32 consumer does;
the analytic gradient the kernel implements; a seeded input generator."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from palettenerf_amd import stylize

REGIMES = {"mild": (1.0, 0.05), "hard": (2.0, 0.3)}      # scale of the raw radiance, scale of the offsets


def make_inputs(M, nb, regime, seed=0, view_dep=False):
    """float64 tensors holding fp32-representable values (so that an fp32 run starts from the very same numbers).
    mild: r ~ N(0,1), offsets ~ 0.05 N, omega = softmax(2 N), palette and target U(0,1).  hard: r ~ 2 N, offsets ~ 0.3 N -- the clamps at 0 and 1
    are active for a real share of the (point, basis, channel) triples."""
    rs, os_ = REGIMES[regime]
    g = torch.Generator().manual_seed(1000 * seed + 17 * M + nb)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    inp = dict(radiance=rs * n(M), offsets=os_ * n(M, nb, 3), omega=torch.softmax(2 * n(M, nb), -1), palette=u(nb, 3), target=u(M, 3))
    inp["view_dep"] = 0.05 * n(M, 3) if view_dep else None
    return {k: None if v is None else v.float().double() for k, v in inp.items()}


def as_fp32(inp, device="cpu"):
    return {k: None if v is None else v.float().to(device).contiguous() for k, v in inp.items()}


def initial_params(nb, dtype=torch.float64):
    return [torch.zeros(nb, dtype=dtype), torch.zeros(nb, 3, dtype=dtype), torch.eye(3, dtype=dtype)[None].repeat(nb, 1, 1)]


def random_params(nb, seed=0):
    """A non-initial point: intensities shifted (some below zero), the transforms away from the identity."""
    g = torch.Generator().manual_seed(77 + seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return [0.5 * n(nb) - 0.3, 0.2 * n(nb, 3), torch.eye(3, dtype=torch.float64)[None] + 0.3 * n(nb, 3, 3)]


def pieces(params, inp):
    dI, dP, dD = params
    s = F.softplus(inp["radiance"])
    pre = s[:, None] + dI[None]                                                   # [M,nb]
    inten = pre.clamp(min=0)
    col = inp["palette"][None] + dP[None] + torch.einsum("npi,pij->npj", inp["offsets"], dD)
    prod = inten[..., None] * col                                                 # [M,nb,3]
    return pre, inten, col, prod


def loss(params, inp, lam):
    """(total loss, regulariser)"""
    dI, dP, dD = params
    _, _, _, prod = pieces(params, inp)
    rgb = (inp["omega"][..., None] * prod.clamp(0, 1)).sum(1)
    if inp["view_dep"] is not None:
        rgb = rgb + inp["view_dep"]
    data = ((rgb - inp["target"]) ** 2).sum()
    E = dD @ dD.transpose(1, 2) - torch.eye(3, dtype=dD.dtype)[None]
    reg = lam * ((E ** 2).sum() + (dP ** 2).sum())
    return data + reg, reg


def autograd_gradient(params, inp, lam):
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    total, reg = loss(ps, inp, lam)
    return list(torch.autograd.grad(total, ps)), total.detach(), reg.detach()


def analytic_gradient(params, inp, lam):
    """The formulas of the kernel: g = 2 e omega [0 <= I C <= 1]; grad dP = sum_n g I + 2 lam dP; grad ddelta = sum_n off (x) g I + 4 lam (D D^T - 1) D;
    grad dI = sum_n [s + dI >= 0] sum_j g C."""
    dI, dP, dD = params
    pre, inten, col, prod = pieces(params, inp)
    rgb = (inp["omega"][..., None] * prod.clamp(0, 1)).sum(1)
    if inp["view_dep"] is not None:
        rgb = rgb + inp["view_dep"]
    e = rgb - inp["target"]
    g = 2 * e[:, None, :] * inp["omega"][..., None] * ((prod >= 0) & (prod <= 1)).to(e.dtype)
    h = g * inten[..., None]
    E = dD @ dD.transpose(1, 2) - torch.eye(3, dtype=dD.dtype)[None]
    return [((pre >= 0).to(e.dtype) * (g * col).sum(-1)).sum(0), h.sum(0) + 2 * lam * dP,
            torch.einsum("npi,npj->pij", inp["offsets"], h) + 4 * lam * (E @ dD)]


def clamp_share(params, inp):
    """Share of the (point, basis, channel) triples at which a clamp cuts: I C outside [0, 1], or s + dI < 0."""
    pre, _, _, prod = pieces(params, inp)
    cut = (prod < 0) | (prod > 1) | (pre < 0)[..., None]
    return float(cut.double().mean())


def sgd(inp, iters, lr=1e-3, momentum=0.9, lam=0.1, total_iters=None, params=None, analytic=False):
    """The float64 loop: returns (params, trace [iters,2] = (loss, regulariser) before each update, momentum buffers).  It runs in the dtype of
    `inp`; analytic=True takes the gradient from the formulas instead of autograd (the seed scan's second fp32 statement, see SEEDS)."""
    dtype = inp["omega"].dtype
    params = [p.clone() for p in (params or initial_params(inp["omega"].shape[1], dtype))]
    lrs = stylize.lr_table(iters, lr, total_iters or max(iters, 1)).astype(np.float32).astype(np.float64)
    bufs, trace = None, torch.zeros(iters, 2, dtype=dtype)
    for t in range(iters):
        if analytic:
            with torch.no_grad():
                grads, (total, reg) = analytic_gradient(params, inp, lam), loss(params, inp, lam)
        else:
            grads, total, reg = autograd_gradient(params, inp, lam)
        trace[t, 0], trace[t, 1] = total, reg
        bufs = grads if bufs is None else [momentum * b + g for b, g in zip(bufs, grads)]
        params = [p - float(lrs[t]) * b for p, b in zip(params, bufs)]
    return params, trace, bufs


# The seed of each long-run case.  A 1000-iteration trajectory amplifies rounding: in the hard regime the deviation of ANY fp32 run from the
# float64 loop is set by the iteration at which some (point, basis, channel) crosses a clamp bound, and two fp32 statements of the same arithmetic
# can land 5x apart on one draw and 1x on the next.  The 4x margin of the GPU tests presumes a draw on which equivalent fp32 formulations agree, so
# the seeds are the first of 0, 1, 2, ... at which, ON THE CPU and without any kernel, (a) the per-op loop's deviation E is <= 2.5e-4, a quarter
# of the validity condition, and (b) this module's analytic-gradient loop in fp32 deviates by between E / 2 and 2 E
# (profiles/stylize/seed_scan.py prints the scan).  Key: (M, nb, regime, view_dep, iters).
SEEDS = {(17, 5, "hard", False, 1000): 1, (64, 4, "hard", False, 1000): 1, (17, 5, "hard", True, 1000): 1}     # every other case: seed 0


@functools.lru_cache(maxsize=None)
def reference_run(M, nb, regime, iters=1000, lr=1e-3, view_dep=False, seed=None):
    """make_inputs(...) and its float64 run with the default hyper-parameters, computed once per session and shared; treat as read-only."""
    if seed is None:
        seed = SEEDS.get((M, nb, regime, view_dep, iters), 0)
    inp = make_inputs(M, nb, regime, seed, view_dep)
    params, trace, bufs = sgd(inp, iters, lr=lr, total_iters=iters)
    return inp, params, trace, bufs


def deviation(params, want):
    """max |x - want| over the three parameter tensors (any shapes that flatten alike), in float64"""
    return max(float((p.detach().double().cpu().reshape(-1) - w.reshape(-1)).abs().max()) for p, w in zip(params, want))
