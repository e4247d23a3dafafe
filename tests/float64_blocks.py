"""The torch statements of three training blocks, written once and evaluated in whatever dtype and on whatever device a test asks for: float64 on the
host is the reference of the unit tests in tests/test_gpu_ops.py; tests/test_gpu_grid_caps.py evaluates the same statements in float64 and in
float32 on the device (the second is the "plain fp32 torch" formulation whose own error against float64 sets the tolerance of a reduced gradient).
Every function takes fp32 tensors, casts detached aliases of them itself (the caller's tensors are left as they are) and returns detached results."""
import torch
import torch.nn.functional as F


def heads_block(h, w_or, b_or, w_om, w1, w2, dtype, device, frozen_h=False):
    """The two colour heads of PaletteNetwork.color (palette/network.py:262-268: Linear with bias; Linear + Softplus, + 0.05, / row sum) and the
    gradients of sum(offrad * w1) + sum(omega * w2).
    -> offrad, omega, [d h (None when frozen), d w_or, d b_or, d w_om], d (omega head's pre-activation) [M, nb]"""
    hh, a, b, c = [t.detach().to(device=device, dtype=dtype).requires_grad_(not (frozen_h and k == 0)) for k, t in enumerate((h, w_or, b_or, w_om))]
    offrad = F.linear(hh, a, b)
    z = F.linear(hh, c)
    z.retain_grad()
    om = F.softplus(z) + 0.05
    om = om / om.sum(-1, keepdim=True)
    ((offrad * w1.to(device=device, dtype=dtype)).sum() + (om * w2.to(device=device, dtype=dtype)).sum()).backward()
    return offrad.detach(), om.detach(), [t.grad for t in (hh, a, b, c)], z.grad


SHADE_NAMES = ("omega", "offsets_radiance", "view_dep", "diffuse", "clip_feat", "smooth_norm", "basis_color")


def shade_block(omega, offrad, view_dep, diffuse, clip_feat, smooth, basis, w_rgb, w_all, clip_dim, dtype, device, frozen=False):
    """The training-mode colour-basis composite (palette/renderer.py:344-386) and the gradients of sum(rgbs * w_rgb) + sum(all_buffer * w_all).
    clip_feat / smooth None: zero columns.  -> rgbs, all_buffer, gradients in the order of SHADE_NAMES (None for an absent input)"""
    ts = [omega, offrad, view_dep, diffuse, clip_feat, smooth, basis]
    o, r, vd, df, cf, sm, bc = [None if t is None else t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in ts]
    M, nb = o.shape
    off, rad = r[:, :-1].reshape(M, nb, 3), r[:, -1:].reshape(M, 1, 1)
    bcc = bc[None].clamp(0, 1)
    if frozen:
        bcc = bcc.detach()
    final = F.softplus(rad) * (bcc + off)
    rgbs = (o[..., None] * final).sum(-2) + vd.detach()
    sparsity = o.sum(-1, keepdim=True) / ((o ** 2).sum(-1, keepdim=True) + 1e-6) - 1
    cols = [sparsity, (vd ** 2).sum(-1, keepdim=True), (off ** 2).sum(-1).sum(-1, keepdim=True),
            sm if sm is not None else torch.zeros(M, 1, dtype=dtype, device=device), vd, df + vd, df,
            cf if cf is not None else torch.zeros(M, clip_dim, dtype=dtype, device=device), o]
    all_ref = torch.cat(cols, -1)
    ((rgbs * w_rgb.to(device=device, dtype=dtype)).sum() + (all_ref * w_all.to(device=device, dtype=dtype)).sum()).backward()
    return rgbs.detach(), all_ref.detach(), [None if t is None else t.grad for t in (o, r, vd, df, cf, sm, bc)]


def mlp_ambiguous(x, weights, fact, device, margin=2e-5):
    """Rows with a hidden pre-activation within `margin` of 0 in float64: such a unit may sit on either side of the kink in fp32 and float64, so a
    test gives these rows no output gradient."""
    with torch.no_grad():
        hd = x.detach().to(device=device, dtype=torch.float64)
        zmin = torch.full((hd.shape[0],), 1e9, dtype=torch.float64, device=device)
        for w in weights[:-1]:
            z = hd @ w.detach().to(device=device, dtype=torch.float64).t()
            zmin = torch.minimum(zmin, z.abs().min(dim=1).values)
            hd = fact(z)
    return zmin < margin


def mlp_block(x, weights, wy, fact, out, dtype, device):
    """The fields' layer loop (nerf/network.py:101-106: bias-free Linear layers, `fact` between them, `out` -- None or torch.sigmoid -- on the last)
    and the gradients of sum(y * wy).  -> y, [dx, dw0, dw1, ...]"""
    xd = x.detach().to(device=device, dtype=dtype).requires_grad_(True)
    wd = [w.detach().to(device=device, dtype=dtype).requires_grad_(True) for w in weights]
    h = xd
    for i, w in enumerate(wd):
        h = h @ w.t()
        if i != len(wd) - 1:
            h = fact(h)
    if out is not None:
        h = out(h)
    (h * wy.to(device=device, dtype=dtype)).sum().backward()
    return h.detach(), [xd.grad] + [w.grad for w in wd]
