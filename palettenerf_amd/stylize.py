"""Fitting a Stylizer: the "optimize" button of the reference's viewer (palette/gui.py:153-194).

The user picks M points of the scene (the `xyz` map of pipeline.viewer_frame) and a colour for each; the field is evaluated there once and
`iters` steps of SGD with momentum fit the Stylizer's dI, dP and ddelta (renderer.Stylizer) to those colours.  On a HIP device the whole
optimisation is ONE launch per 10 000 iterations (pnr_stylizer_fit); `fit_stylizer_per_op` is the same loop as the reference writes it, op by
op, and what runs on CPU tensors, outside the entry's limits, or with `enabled = False`.

    out = pipeline.viewer_frame(model, pose, intrinsics, W, H)          # out["xyz"][v, u] -> a picked point
    model.stylizer = stylize.fit_stylizer(model, points, colors)        # the next gui_mode frame is stylised
"""
import ctypes
import types

import numpy as np
import torch

from . import _lib, renderer
from ._torch_glue import stream_ptr

enabled = True      # False: always the per-op loop (A/B measurements, tests)

_UNSUPPORTED = -2   # PNR_ERR_UNSUPPORTED


def lr_table(iters, lr=1e-3, total_iters=1000, first_iter=0):
    """The learning rate of iterations first_iter .. first_iter + iters - 1 as float64: lr * 0.1 ** min(t / total_iters, 1), the values
    LambdaLR yields at palette/gui.py:173, evaluated as Python doubles exactly as the scheduler does.  The consumer narrows to fp32 once."""
    return np.array([lr * 0.1 ** min(t / total_iters, 1) for t in range(int(first_iter), int(first_iter) + int(iters))], dtype=np.float64)


def stylizer_inputs(model, points):
    """The field at the picked points as the optimisation sees it (palette/gui.py:157-167): the model's own forward(points, zeros) under no_grad.
    Returns radiance [M], omega [M,nb], offsets [M,nb,3], palette [nb,3] (basis_color clamped to [0, 1])."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("stylizer_inputs: points must be an [M, 3] float32 tensor")
    nb, M = int(model.num_basis), points.shape[0]
    with torch.no_grad():
        _, _, omega, offsets_radiance, _, _ = model(points, torch.zeros_like(points))
        radiance = offsets_radiance[..., -1].reshape(M).contiguous()
        offsets = offsets_radiance[..., :-1].reshape(M, nb, 3).contiguous()
        omega = omega.reshape(M, nb).contiguous()
        palette = model.basis_color.detach().clamp(0, 1).reshape(nb, 3).contiguous()
    return radiance, omega, offsets, palette


def _params(stylizer):
    return [stylizer.dI, stylizer.dP, stylizer.ddelta]


def fit_stylizer_per_op(stylizer, radiance, omega, offsets, palette, colors, iters, lr=1e-3, momentum=0.9, lambda_arap=0.1, total_iters=1000,
                        first_iter=0, buffers=None, view_dep=None, want_trace=False):
    """The loop of palette/gui.py:169-187 on `stylizer`, in place: torch.optim.SGD with momentum and LambdaLR over Stylizer.forward and
    ARAP_loss.  `buffers` (three tensors) continue a run; returns (buffers after the run, trace [iters,2] or None)."""
    params = _params(stylizer)
    optimizer = torch.optim.SGD(params, lr=lr, momentum=momentum)
    if buffers is not None:
        for p, b in zip(params, buffers):
            optimizer.state[p]["momentum_buffer"] = b.detach().clone().reshape(p.shape)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda it: 0.1 ** min((it + first_iter) / total_iters, 1))
    rows = []
    for _ in range(int(iters)):
        optimizer.zero_grad()
        rgbs = stylizer(radiance, omega, palette, offsets, view_dep)
        loss = ((rgbs - colors) ** 2).sum()
        loss_arap = stylizer.ARAP_loss() * lambda_arap
        loss_arap = loss_arap + (stylizer.dP ** 2).sum() * lambda_arap
        loss = loss + loss_arap
        loss.backward()
        optimizer.step()
        scheduler.step()
        if want_trace:
            rows.append(torch.stack([loss.detach(), loss_arap.detach()]))
    for p in params:
        p.grad = None
    out = [optimizer.state[p].get("momentum_buffer") for p in params]
    out = [torch.zeros_like(p) if b is None else b.detach().reshape(p.shape) for p, b in zip(params, out)]
    trace = None
    if want_trace:
        trace = torch.stack(rows) if rows else torch.zeros(0, 2, dtype=torch.float32, device=radiance.device)
    return out, trace


def _fit_launch(stylizer, radiance, omega, offsets, palette, colors, iters, lr, momentum, lambda_arap, total_iters, first_iter, buffers, view_dep,
                want_trace):
    """pnr_stylizer_fit, one launch per 10 000 iterations.  Returns None when the entry answers PNR_ERR_UNSUPPORTED (nothing has run then)."""
    device, M, nb = radiance.device, radiance.shape[0], omega.shape[1]
    params = _params(stylizer)
    fresh = buffers is None
    buffers = [torch.zeros_like(p) for p in params] if fresh else [b.detach().clone().reshape(p.shape).contiguous() for p, b in zip(params, buffers)]
    lrs = torch.from_numpy(lr_table(iters, lr, total_iters, first_iter).astype(np.float32)).to(device)
    trace = torch.empty(iters, 2, dtype=torch.float32, device=device) if want_trace else None
    fn = _lib.load().pnr_stylizer_fit
    with torch.cuda.device(device):
        for c0 in range(0, iters, _lib.STYLIZER_MAX_ITERS):
            n = min(_lib.STYLIZER_MAX_ITERS, iters - c0)
            a = _lib.StylizerFitArgs(M=M, num_basis=nb, iters=n, radiance=radiance.data_ptr(), omega=omega.data_ptr(), offsets=offsets.data_ptr(),
                                     palette=palette.data_ptr(), target=colors.data_ptr(), view_dep=None if view_dep is None else view_dep.data_ptr(),
                                     dI=params[0].data_ptr(), dP=params[1].data_ptr(), ddelta=params[2].data_ptr(), mom_dI=buffers[0].data_ptr(),
                                     mom_dP=buffers[1].data_ptr(), mom_ddelta=buffers[2].data_ptr(), has_momentum=int(not fresh or c0 > 0),
                                     lr=lrs.data_ptr() + 4 * c0, momentum=momentum, lambda_arap=lambda_arap,
                                     trace=None if trace is None else trace.data_ptr() + 8 * c0)
            rc = fn(ctypes.byref(a), stream_ptr())
            if rc == _UNSUPPORTED and c0 == 0:
                return None
            _lib.check(rc, "pnr_stylizer_fit")
    for p in params:
        torch.autograd.graph.increment_version(p)     # written by a raw kernel: the edit blob (fused.py) is keyed on the version counters
    return buffers, trace


def _check(name, t, shape, device):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"fit_stylizer: {name} must be a float32 tensor of shape {tuple(shape)}, got {got}")
    if t.device != device:
        raise ValueError(f"fit_stylizer: {name} is on {t.device}, the other inputs on {device}")
    return t.detach().contiguous()


def fit_stylizer_from_inputs(radiance, omega, offsets, palette, colors, iters=1000, lr=1e-3, momentum=0.9, lambda_arap=0.1, total_iters=None,
                             stylizer=None, state=None, return_trace=False, view_dep=None, opt=None):
    """fit_stylizer on the tensors stylizer_inputs returns (any source of them will do).  view_dep [M,3] is added to the colour as a constant
    (palette/renderer.py:181-182); the viewer passes none."""
    if not torch.is_tensor(omega) or omega.dim() != 2:
        raise ValueError("fit_stylizer: omega must be an [M, num_basis] float32 tensor")
    M, nb = omega.shape
    device = omega.device
    if M == 0:
        raise ValueError("fit_stylizer: no points")
    if not torch.is_tensor(colors):
        colors = torch.as_tensor(np.asarray(colors), dtype=torch.float32).to(device)
    if torch.is_tensor(radiance) and radiance.dim() != 1 and radiance.numel() == M:
        radiance = radiance.reshape(M)
    radiance, omega, offsets = _check("radiance", radiance, (M,), device), _check("omega", omega, (M, nb), device), _check("offsets", offsets, (M, nb, 3), device)
    if torch.is_tensor(palette) and palette.dim() == 3 and palette.shape[0] == 1:
        palette = palette[0]
    palette, colors = _check("palette", palette, (nb, 3), device), _check("colors", colors, (M, 3), device)
    if view_dep is not None:
        view_dep = _check("view_dep", view_dep, (M, 3), device)
    iters = int(iters)
    if iters < 0 or not (lr >= 0) or not (0 <= momentum) or (total_iters is not None and total_iters < 1):
        raise ValueError("fit_stylizer: iters, lr and momentum must not be negative, total_iters at least 1")
    if stylizer is None:
        stylizer = renderer.Stylizer(opt if opt is not None else types.SimpleNamespace(num_basis=nb)).to(device)
    else:
        for name, p, shape in (("dI", stylizer.dI, (nb,)), ("dP", stylizer.dP, (1, nb, 3)), ("ddelta", stylizer.ddelta, (nb, 3, 3))):
            _check("stylizer." + name, p, shape, device)
            if not p.is_contiguous():
                raise ValueError(f"fit_stylizer: stylizer.{name} must be contiguous")
    first_iter, buffers = 0, None
    if state is not None:
        first_iter, buffers = int(state["iters"]), list(state["momentum"])
        if len(buffers) != 3:
            raise ValueError("fit_stylizer: state['momentum'] holds the three buffers of dI, dP and ddelta")
        for name, b, p in zip(("dI", "dP", "ddelta"), buffers, _params(stylizer)):
            _check("state momentum of " + name, b, p.shape, device)
        if total_iters is None:
            total_iters = state["total_iters"]
    if total_iters is None:
        total_iters = max(iters, 1)
    total_iters = int(total_iters)
    done = None
    if iters == 0:
        done = (buffers if buffers is not None else [torch.zeros_like(p) for p in _params(stylizer)],
                torch.zeros(0, 2, dtype=torch.float32, device=device) if return_trace else None)
    elif enabled and device.type == "cuda":
        done = _fit_launch(stylizer, radiance, omega, offsets, palette, colors, iters, float(lr), float(momentum), float(lambda_arap), total_iters,
                           first_iter, buffers, view_dep, return_trace)
    if done is None:
        done = fit_stylizer_per_op(stylizer, radiance, omega, offsets, palette, colors, iters, float(lr), float(momentum), float(lambda_arap),
                                   total_iters, first_iter, buffers, view_dep, return_trace)
    if not return_trace:
        return stylizer
    return stylizer, done[1], {"momentum": tuple(done[0]), "iters": first_iter + iters, "total_iters": total_iters}


def fit_stylizer(model, points, colors, iters=1000, lr=1e-3, momentum=0.9, lambda_arap=0.1, total_iters=None, stylizer=None, state=None,
                 return_trace=False):
    """The reference's optimisation (palette/gui.py:153-194; its defaults) for the points [M,3] picked in the scene and their colours [M,3]:
    returns a renderer.Stylizer on the model's device, ready for `model.stylizer = ...`.  `stylizer=` continues from an existing module (in
    place), otherwise dI = 0, dP = 0, ddelta = identity.  The learning rate of iteration t is lr * 0.1 ** min(t / total_iters, 1); total_iters
    defaults to the state's, else to iters.  With return_trace: (stylizer, trace [iters,2] = (loss, regulariser) before each update, state);
    `state` holds the momentum buffers and the iteration count, so that fit(600, total_iters=1000) followed by fit(400, stylizer=, state=)
    is fit(1000).  Shape or dtype mismatches raise ValueError before anything runs."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("fit_stylizer: points must be an [M, 3] float32 tensor")
    device = next(model.parameters()).device
    M = points.shape[0]
    if not torch.is_tensor(colors):
        colors = torch.as_tensor(np.asarray(colors), dtype=torch.float32)
    if tuple(colors.shape) != (M, 3) or colors.dtype != torch.float32:
        raise ValueError(f"fit_stylizer: colors must be a float32 array of shape {(M, 3)}, got {tuple(colors.shape)} {colors.dtype}")
    if M == 0:
        raise ValueError("fit_stylizer: no points")
    radiance, omega, offsets, palette = stylizer_inputs(model, points.to(device))
    return fit_stylizer_from_inputs(radiance, omega, offsets, palette, colors.to(device), iters, lr, momentum, lambda_arap, total_iters, stylizer,
                                    state, return_trace, opt=model.opt)
