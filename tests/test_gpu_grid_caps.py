"""The tiled kernels past their grid caps, where a workgroup walks more than one tile (`for (t = blockIdx.x; t < ntiles; t += gridDim.x)`): on its
second trip a kernel reuses its LDS tile behind its own barriers, recomputes row0 / nrows and carries register state (the shade backward's
basis-colour accumulator, the MLPs' weight-gradient accumulators and per-tile scaling) from the first.  The families' unit tests all run below the caps.

Every test takes its batch from pnr_launch_geometry: with K = cap x rows_per_trip the batch is M = K + 2 x rows_per_trip + 3, so that workgroups 0
and 1 take a full second tile, workgroup 2 a ragged one of 3 rows and every other workgroup stops after one -- and asserts from the query that the
second trip happens (a raised cap fails the test instead of emptying it).  Three kinds of assertion:
 (a) row-wise outputs, bit for bit: f(x)[:K] == f(x[:K]) and f(x)[K:] == f(x[K:]) -- K is a multiple of every tile, so the second-trip rows of the
     full launch are first-trip rows of the fresh one;
 (b) the second-trip rows against the float64 statement of the family's unit test, at that test's tolerances (per-row quantities do not depend on M);
 (c) quantities reduced over all rows (basis-colour gradient, MLP and head weight gradients) against float64 over the full batch: the tolerance is
     4 x the error of the same reduction in plain fp32 torch on the device at this batch (the rule of tests/test_gpu_smooth.py) + one fp32 ulp of
     the largest entry; two runs give the same bits.  The figures measured on an MI355X are in profiles/grid_caps/README.md."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from palettenerf_amd import _lib, palette_utils, scene
from palettenerf_amd._torch_glue import call, ptr
from tests import float64_blocks as f64
from tests import test_gpu_smooth as S

pytestmark = pytest.mark.gpu

FAR = 1 << 31
u32 = ctypes.c_uint32


def batch_past(*entries):
    """(K, M) for the entries of one family: K = the largest cap x tile among them, M = K + 2 tiles + 3 rows; asserts that the tiles coincide at K
    and, from the query at M itself, that every entry takes a second trip."""
    caps = {e: _lib.launch_geometry(e, FAR) for e in entries}
    rpt = max(r for _, r in caps.values())
    K = max(w * r for w, r in caps.values())
    M = K + 2 * rpt + 3
    for e, (w, r) in caps.items():
        assert K % (w * r) == 0 and rpt % r == 0, (e, w, r)
        wg, r2 = _lib.launch_geometry(e, M)
        assert M > wg * r2, f"{e}: {M} rows fit one trip of {wg} workgroups x {r2} rows -- the cap moved and this test no longer reaches the second trip"
        print(f"{e}: {wg} workgroups x {r2} rows per trip; batch {M} = {K} + 2 x {rpt} + 3")
    return K, M


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    assert torch.equal(bits(a), bits(b)), (what, int((bits(a) != bits(b)).sum()), "elements differ")


def aligned(*ts):
    for t in ts:
        assert t is None or t.data_ptr() % 16 == 0


def slices_agree(full, head, tail, K, what):
    """(a) for one family: dicts of row-wise outputs of the full launch, of the launch on rows [:K] and of the launch on rows [K:]."""
    for k in full:
        if full[k] is None:
            assert head[k] is None and tail[k] is None
            continue
        same_bits(full[k][:K], head[k], (what, k, "first trip"))
        same_bits(full[k][K:], tail[k], (what, k, "second trip"))


def close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=str(what))


def grad_close(got, want, what):
    """The unit tests' bound for a per-row gradient: 2e-5 of the tensor's largest entry (+ 1e-7)."""
    scale = float(want.abs().max()) + 1e-12
    err = float((got.double() - want).abs().max())
    print(f"{what}: max err {err:.3e} of max {scale:.3e}")
    assert err <= 2e-5 * scale + 1e-7, (what, err, scale)


def reduced_close(got, ref64, torch32, what):
    """(c): |got - float64| <= 4 x (largest error of the fp32 torch formulation at this batch) + one fp32 ulp of the largest entry."""
    scale = float(ref64.abs().max())
    err32 = float((torch32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    tol = 4 * err32 + float(np.spacing(np.float32(scale)))
    print(f"{what}: max |g| {scale:.4e}  fused err {err:.3e} ({err / scale:.3e} of max)  fp32-torch err {err32:.3e} ({err32 / scale:.3e} of max)  tol {tol:.3e}")
    assert scale > 0 and err <= tol, (what, err, err32, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------- heads
def test_palette_heads_past_the_grid_cap(cuda):
    nb, n_in = 4, 15
    orw = 3 * nb + 1
    K, M = batch_past("pnr_palette_heads_forward", "pnr_palette_heads_backward")
    g = torch.Generator(device=cuda).manual_seed(101)
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)      # noqa: E731
    h = rn(M, n_in)
    h[K:K + 40] *= torch.linspace(5.0, 30.0, 40, device=cuda)[:, None]       # second-trip rows beyond F.softplus' threshold (20)
    w_or, b_or, w_om = rn(orw, n_in) * 0.3, rn(orw) * 0.1, rn(nb, n_in) * 0.5
    w1, w2 = rn(M, orw), rn(M, nb)

    def run(lo, hi):
        hs, g1, g2 = h[lo:hi], w1[lo:hi], w2[lo:hi]
        aligned(hs, g1, g2)
        n = hi - lo
        offrad, omega = torch.empty(n, orw, device=cuda), torch.empty(n, nb, device=cuda)
        grad_h, grad_pre = torch.empty(n, n_in, device=cuda), torch.empty(n, orw + nb, device=cuda)
        call("pnr_palette_heads_forward", ptr(hs), ptr(w_or), ptr(b_or), ptr(w_om), u32(n), u32(nb), u32(n_in), ptr(offrad), ptr(omega))
        call("pnr_palette_heads_backward", ptr(hs), ptr(w_or), ptr(w_om), ptr(g1), ptr(g2), u32(n), u32(nb), u32(n_in), ptr(grad_h), ptr(grad_pre))
        return dict(offsets_radiance=offrad, omega=omega, grad_h=grad_h, grad_pre=grad_pre)

    full, head, tail = run(0, M), run(0, K), run(K, M)
    slices_agree(full, head, tail, K, "heads")
    # (b) the second-trip rows against the float64 formulas
    offrad64, om64, grads64, gz64 = f64.heads_block(h[K:], w_or, b_or, w_om, w1[K:], w2[K:], torch.float64, cuda)
    close(full["offsets_radiance"][K:], offrad64, 2e-6, 2e-5, "offsets_radiance")
    close(full["omega"][K:], om64, 2e-6, 2e-6, "omega")
    grad_close(full["grad_h"][K:], grads64[0], "heads grad_h, second-trip rows")
    same_bits(full["grad_pre"][K:, :orw], w1[K:], "grad_pre: the offsets_radiance head's part is its output gradient")
    grad_close(full["grad_pre"][K:, orw:], gz64, "heads grad_pre (omega head), second-trip rows")
    # (c) the weight and bias gradients of the full batch, through the autograd function (pnr_linear_wgrad / pnr_linear_bgrad over grad_pre)
    _, _, ref, _ = f64.heads_block(h, w_or, b_or, w_om, w1, w2, torch.float64, cuda)
    _, _, t32, _ = f64.heads_block(h, w_or, b_or, w_om, w1, w2, torch.float32, cuda)

    def fused():
        leaves = [t.detach().clone().requires_grad_(True) for t in (h, w_or, b_or, w_om)]
        offrad, omega = palette_utils._palette_heads.apply(*leaves)
        torch.autograd.backward([offrad, omega], [w1, w2])
        same_bits(offrad.detach(), full["offsets_radiance"], "the autograd function launches the same forward")
        same_bits(leaves[0].grad, full["grad_h"], "... and the same backward")
        return [t.grad for t in leaves]

    first, second = fused(), fused()
    for k, name in ((1, "w_offsets_radiance"), (2, "b_offsets_radiance"), (3, "w_omega")):
        reduced_close(first[k], ref[k], t32[k], f"heads d {name}, {M} rows")
        same_bits(first[k], second[k], (name, "two runs"))


# --------------------------------------------------------------------------------------------------------------------------------------- smooth
SMOOTH_SHAPE = (4, "clip16_sigma0.5")


@pytest.fixture(scope="module")
def smooth_case(cuda):
    K, M = batch_past("pnr_palette_smooth_forward", "pnr_palette_smooth_backward")
    c = S.case.__wrapped__(M, *SMOOTH_SHAPE)         # (not through the cache: half a million rows are let go with this module)
    t = {k: None if v is None else v.cuda() for k, v in c["inputs"].items()}
    nb, clip_dim = SMOOTH_SHAPE[0], S.CLIPS[SMOOTH_SHAPE[1]][0]

    def forward(lo, hi):
        a = [None if t[k] is None else t[k][lo:hi] for k in S.NAMES]
        aligned(*a)
        w, n = torch.empty(hi - lo, device=cuda), torch.empty(hi - lo, device=cuda)
        call("pnr_palette_smooth_forward", hi - lo, nb, clip_dim, *[ptr(v) for v in a], float(c["bound"]), S.SIGMA_XYZ, S.SIGMA_COLOR, c["sigma_clip"],
             ptr(w), ptr(n))
        return dict(smooth_weight=w, smooth_norm=n)

    return dict(K=K, M=M, c=c, t=t, nb=nb, clip_dim=clip_dim, forward=forward, full=forward(0, M))


def test_palette_smooth_forward_past_the_grid_cap(cuda, smooth_case):
    s = smooth_case
    K, M = s["K"], s["M"]
    slices_agree(s["full"], s["forward"](0, K), s["forward"](K, M), K, "smooth forward")
    tail = S.rows_of(s["c"], K, M)
    for name in ("smooth_norm", "smooth_weight"):
        S.check(name, s["full"][name][K:].view(-1, 1), tail, ("second-trip rows", M) + SMOOTH_SHAPE)
    same = tail["same"].cuda()
    assert bool(same.any()) and bool((s["full"]["smooth_norm"][K:][same] == 0).all())         # an equal pair: exactly no change


def test_palette_smooth_backward_past_the_grid_cap(cuda, smooth_case):
    s = smooth_case
    K, M, t, c = s["K"], s["M"], s["t"], s["c"]
    g_norm, weight = c["g_norm"].cuda().view(-1), s["full"]["smooth_weight"]

    def backward(lo, hi):
        ins = [g_norm[lo:hi], weight[lo:hi]] + [t[k][lo:hi] for k in S.GRAD_NAMES]
        aligned(*ins)
        outs = [torch.empty_like(t[k][lo:hi]) for k in S.GRAD_NAMES]
        call("pnr_palette_smooth_backward", hi - lo, s["nb"], s["clip_dim"], *[ptr(v) for v in ins], *[ptr(v) for v in outs])
        return {"grad_" + k: v for k, v in zip(S.GRAD_NAMES, outs)}

    full = backward(0, M)
    slices_agree(full, backward(0, K), backward(K, M), K, "smooth backward")
    tail = S.rows_of(c, K, M)
    for name in full:
        assert torch.isfinite(full[name]).all(), name
        S.check(name, full[name][K:], tail, ("second-trip rows", M) + SMOOTH_SHAPE)
    same_bits(full["grad_omega"], -full["grad_omega_diff"], "the pair's gradients are each other's negation")
    same_bits(full["grad_clip_feat"], -full["grad_clip_feat_diff"], "the pair's gradients are each other's negation")


@pytest.mark.parametrize("start", ["aligned", "unaligned"])
def test_palette_smooth_points_past_the_grid_cap(cuda, start):
    """pnr_palette_smooth_points counts what a lane handles per trip: float4 groups (3 M / 4) when its arrays start on 16-byte boundaries, single
    elements (3 M) otherwise.  The batch puts K + 2 x 256 + 3 of them in the launch; the rows from `split` on lie wholly in the second trip."""
    bound = 2
    cap, rpt = _lib.launch_geometry("pnr_palette_smooth_points", FAR)
    K = cap * rpt
    items = K + 2 * rpt + 3
    if start == "aligned":
        M = -(-4 * items // 3)
        n_items, split = 3 * M // 4, 4 * (-(-K // 3) + 1)     # row r's first element sits in group 3 r / 4 >= K; a multiple of 4 rows is 48 bytes
    else:
        M = -(-items // 3)
        n_items, split = 3 * M, -(-K // 3) + 1
        split += (split + 1) % 4 == 0                          # the slice x[1:][split:] must not start on a 16-byte boundary either
    wg, r2 = _lib.launch_geometry("pnr_palette_smooth_points", n_items)
    print(f"pnr_palette_smooth_points ({start}): {wg} workgroups x {r2} lanes; {M} rows = {n_items} items, second trip from row {split}")
    assert n_items >= items and n_items > wg * r2, "the cap moved: no second trip at this batch"
    assert 3 * split // (4 if start == "aligned" else 1) >= K and split < M
    g = torch.Generator(device=cuda).manual_seed(7)
    pad = 0 if start == "aligned" else 1
    xyzs_p, noise_p = torch.zeros(M + pad, 3, device=cuda), torch.zeros(M + pad, 3, device=cuda)
    xyzs, noise = xyzs_p[pad:], noise_p[pad:]
    xyzs[:] = (torch.rand(M, 3, device=cuda, generator=g) * 2 - 1) * bound
    xyzs[::3, 0] = bound * (1 - 0.03 * torch.rand(xyzs[::3].shape[0], device=cuda, generator=g))     # the clamp acts on most of these
    xyzs[1::4, 1] = -bound
    xyzs[2::7, 2] = bound
    noise[:] = torch.rand(M, 3, device=cuda, generator=g)
    noise[::5] = noise[::5].round()              # draws of exactly 0 (rand's range includes it) and the supremum
    noise[split + (1 - split) % 4] = 0           # ... one of them at a second-trip sample that sits on -bound
    for lo in (0, split):
        assert (xyzs[lo:].data_ptr() % 16 == 0) == (start == "aligned") and (noise[lo:].data_ptr() % 16 == 0) == (start == "aligned")
    want = (xyzs + noise * bound * 0.03).clamp(-bound, bound)
    assert bool((want[split:] == bound).any() and (want[split:] == -bound).any())
    full = palette_utils.smooth_points(xyzs, noise, bound)
    assert torch.equal(full, want)
    same_bits(full[:split], palette_utils.smooth_points(xyzs[:split], noise[:split], bound), "first trip")
    same_bits(full[split:], palette_utils.smooth_points(xyzs[split:], noise[split:], bound), "second trip")


# ---------------------------------------------------------------------------------------------------------------------------------------- shade
def test_palette_train_shade_past_the_grid_caps(cuda):
    """One batch past the forward's cap (4096 workgroups) is eight trips deep for the backward (512), whose basis-colour accumulator lives in
    registers across a workgroup's tiles."""
    nb, clip_dim = 4, 16
    K, M = batch_past("pnr_palette_train_shade_forward", "pnr_palette_train_shade_backward")
    g = torch.Generator(device=cuda).manual_seed(202)
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)      # noqa: E731
    ru = lambda *s: torch.rand(*s, device=cuda, generator=g)       # noqa: E731
    omega = F.softplus(rn(M, nb)) + 0.05
    omega = omega / omega.sum(-1, keepdim=True)
    offrad = rn(M, 3 * nb + 1) * 0.5
    offrad[K:K + 50, -1] = torch.linspace(15.0, 30.0, 50, device=cuda)       # second-trip rows around F.softplus' threshold (20)
    view_dep, diffuse, clip_feat, smooth = ru(M, 3), ru(M, 3), rn(M, clip_dim), ru(M, 1)
    basis = torch.tensor([[0.2, 0.5, 1.15], [-0.1, 0.9, 0.4], [0.7, 0.0, 1.0], [0.35, 1.2, -0.05]], device=cuda)     # some components outside [0, 1]
    outside = (basis < 0) | (basis > 1)
    assert basis.shape == (nb, 3) and int(outside.sum()) == 4
    w_rgb, w_all = rn(M, 3), rn(M, 13 + clip_dim + nb)
    rows = (omega, offrad, view_dep, diffuse, clip_feat, smooth)

    def run(lo, hi):
        leaves = [t[lo:hi].detach().requires_grad_(True) for t in rows] + [basis.clone().requires_grad_(True)]
        aligned(*leaves, w_rgb[lo:hi], w_all[lo:hi])
        rgbs, all_buffer = palette_utils.palette_train_shade(*leaves, clip_dim)
        torch.autograd.backward([rgbs, all_buffer], [w_rgb[lo:hi], w_all[lo:hi]])
        out = dict(rgbs=rgbs.detach(), all_buffer=all_buffer.detach())
        out.update({"grad_" + n: t.grad for n, t in zip(f64.SHADE_NAMES[:6], leaves)})
        return out, leaves[6].grad

    (full, g_basis), (head, _), (tail, _) = run(0, M), run(0, K), run(K, M)
    assert full["all_buffer"].shape == (M, 13 + clip_dim + nb) and full["grad_smooth_norm"].shape == (M, 1)
    slices_agree(full, head, tail, K, "shade")
    # (b) the second-trip rows against the float64 formulas
    rgbs64, all64, grads64 = f64.shade_block(*[t[K:] for t in rows], basis, w_rgb[K:], w_all[K:], clip_dim, torch.float64, cuda)
    close(full["rgbs"][K:], rgbs64, 2e-6, 2e-6, "rgbs")
    close(full["all_buffer"][K:], all64, 2e-6, 2e-6, "all_buffer")
    for name, want in zip(f64.SHADE_NAMES[:6], grads64):
        grad_close(full["grad_" + name][K:], want, f"shade grad {name}, second-trip rows")
    # (c) the basis-colour gradient: per-thread registers across the tiles -> wave shuffle -> LDS -> one partial row per workgroup -> fixed-order sum
    ref = f64.shade_block(*rows, basis, w_rgb, w_all, clip_dim, torch.float64, cuda)[2][6]
    t32 = f64.shade_block(*rows, basis, w_rgb, w_all, clip_dim, torch.float32, cuda)[2][6]
    reduced_close(g_basis, ref, t32, f"shade d basis_color, {M} rows")
    assert float(g_basis[outside].abs().max()) == 0.0 and float(ref[outside].abs().max()) == 0.0       # the clamp passes nothing there
    assert bool((g_basis[~outside] != 0).all())
    same_bits(g_basis, run(0, M)[1], "two runs")


# ---------------------------------------------------------------------------------------------------------------------------- field and density
def nerf_model(cuda, seed):
    from palettenerf_amd import network
    m = network.NeRFNetwork(bound=2, cuda_ray=True)
    scene.seed_field_(m, seed)
    return m.to(cuda).eval()


def sample_points(cuda, M, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    x = torch.rand(M, 3, device=cuda, generator=g) * 4 - 2
    d = F.normalize(torch.randn(M, 3, device=cuda, generator=g), dim=-1)
    return x, d


@pytest.mark.parametrize("precision", [0, 1, 2])      # PNR_FIELD_FP32 / PNR_FIELD_F16X3 / PNR_FIELD_F16X2
def test_nerf_field_past_the_grid_cap(cuda, precision):
    import oracle
    from palettenerf_amd.fused import NeRFFieldFused
    K, M = batch_past("pnr_nerf_field_forward")
    m = nerf_model(cuda, 3)
    field = NeRFFieldFused(m)
    field.precision = precision
    assert field.effective_precision() == precision
    x, d = sample_points(cuda, M, 50 + precision)

    def run(lo, hi):
        aligned(x[lo:hi], d[lo:hi])
        sigmas, rgbs = field(x[lo:hi], d[lo:hi])
        return dict(sigmas=sigmas, rgbs=rgbs)

    full = run(0, M)
    slices_agree(full, run(0, K), run(K, M), K, f"nerf field, precision {precision}")
    # (b) the second-trip rows against the torch modules and the oracle's sequential fp32 chains, at the unit tests' bounds
    host = lambda t: t.detach().cpu().numpy()      # noqa: E731
    s, c = host(full["sigmas"][K:]), host(full["rgbs"][K:])
    xt, dt = host(x[K:]), host(d[K:])
    enc = oracle.grid_encode_forward((xt + 2) / 4, host(m.encoder.embeddings), host(m.encoder.offsets), m.encoder.per_level_scale, 16)
    so, co = oracle.nerf_field_forward(enc, dt, *[host(l.weight) for l in list(m.sigma_net) + list(m.color_net)])
    if precision == 2:      # colours with activations rounded once to fp16: inside the 5e-5 contract; sigma as the split form
        err_c, err_s = np.abs(c - co).max(), np.abs(s / so - 1).max()
        print(f"f16x2 second-trip rows: colour err {err_c:.3e}, sigma rel err {err_s:.3e}")
        assert err_c < 5e-5 and err_s < 2e-5, (err_c, err_s)
        return
    with torch.no_grad():
        m.fused_field = False
        s_ref, c_ref = m(x[K:], d[K:])
    for want_s, want_c in ((host(s_ref), host(c_ref)), (so, co)):
        np.testing.assert_allclose(s, want_s, rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(c, want_c, rtol=0, atol=2e-6)


@pytest.mark.parametrize("precision", [0, 1])
def test_nerf_density_past_the_grid_cap(cuda, precision):
    from palettenerf_amd.fused import DensityFused
    K, M = batch_past("pnr_nerf_density_forward")
    m = nerf_model(cuda, 5)
    density = DensityFused(m)
    density.precision = precision
    assert density.effective_precision() == precision
    x, _ = sample_points(cuda, M, 60 + precision)

    def run(lo, hi):
        aligned(x[lo:hi])
        sigmas, geo = density(x[lo:hi])
        return dict(sigmas=sigmas, geo_feat=geo)

    full = run(0, M)
    slices_agree(full, run(0, K), run(K, M), K, f"density, precision {precision}")
    with torch.no_grad():
        want = m.density(x[K:])                      # fused_field is off: torch modules over the HIP encoder
    close(full["sigmas"][K:], want["sigma"], 2e-5, 1e-30, "sigma")
    close(full["geo_feat"][K:], want["geo_feat"], 0, 2e-5, "geo_feat")


# ------------------------------------------------------------------------------------------------------------------------------------------ MLP
@pytest.mark.parametrize("f16x3", [0, 1])        # exact fp32 matrix instructions (k_mlp_fwd / k_mlp_bwd) / split-fp16 products (k_mlp_fwd_h / k_mlp_bwd_h)
def test_fused_mlp_past_the_grid_caps(cuda, f16x3, monkeypatch):
    """The colour net's stack.  One batch past the forward's cap (512 workgroups) is past the backward's (256), whose weight-gradient accumulators
    stay in registers over a workgroup's tiles."""
    from palettenerf_amd import mlp
    dims = (31, 64, 64, 3)
    K, M = batch_past("pnr_mlp_forward", "pnr_mlp_backward")
    monkeypatch.setattr(mlp, "MIN_ROWS", 1)          # the fresh launch on the second-trip rows alone is a small batch
    torch.manual_seed(sum(dims))
    net = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1], bias=False) for i in range(len(dims) - 1)]).to(cuda)
    for l in net:
        torch.nn.init.normal_(l.weight, std=1.0 / l.in_features ** 0.5)
    weights = [l.weight for l in net]
    x, wy = torch.randn(M, dims[0], device=cuda), torch.randn(M, dims[-1], device=cuda)
    ambiguous = f64.mlp_ambiguous(x, weights, F.relu, cuda, margin=2e-5)      # a hidden unit on the kink: no output gradient for that row
    assert int(ambiguous.sum()) < 2000
    wy[ambiguous] = 0.0

    def run(lo, hi):
        xs = x[lo:hi].detach().requires_grad_(True)
        aligned(xs, wy[lo:hi])
        for l in net:
            l.weight.grad = None
        assert mlp.fusable(net, xs, F.relu)
        y = mlp.run_mlp(net, xs, F.relu, None)
        assert type(y.grad_fn).__name__.startswith("_FusedMLP")
        y.backward(wy[lo:hi])
        return dict(y=y.detach(), dx=xs.grad), [l.weight.grad.clone() for l in net]

    lib = _lib.load()
    try:
        assert lib.pnr_set_option(b"mlp_f16x3", f16x3) == 0
        (full, dws), (head, _), (tail, _) = run(0, M), run(0, K), run(K, M)
        dws_again = run(0, M)[1]
    finally:
        lib.pnr_set_option(b"mlp_f16x3", 1)
        for l in net:
            l.weight.grad = None
    slices_agree(full, head, tail, K, f"mlp, f16x3 {f16x3}")
    # (b) the second-trip rows against the layer loop in float64
    y64, g64 = f64.mlp_block(x[K:], weights, wy[K:], F.relu, None, torch.float64, cuda)
    scale = float(y64.abs().max())
    err = float((full["y"][K:].double() - y64).abs().max())
    print(f"mlp y, second-trip rows: max err {err:.3e} of max {scale:.3e}")
    assert err <= 2e-6 * scale
    err, ref = float((full["dx"][K:].double() - g64[0]).abs().max()), float(g64[0].abs().max())
    print(f"mlp dx, second-trip rows: max err {err:.3e} of max {ref:.3e}")
    assert err <= 2e-5 * ref
    # (c) the weight gradients of the full batch (register accumulators -> LDS over the waves -> one partial row per workgroup -> k_mlp_dw_reduce)
    ref = f64.mlp_block(x, weights, wy, F.relu, None, torch.float64, cuda)[1][1:]
    t32 = f64.mlp_block(x, weights, wy, F.relu, None, torch.float32, cuda)[1][1:]
    for l, (got, again) in enumerate(zip(dws, dws_again)):
        reduced_close(got, ref[l], t32[l], f"mlp dw{l}, f16x3 {f16x3}, {M} rows")
        same_bits(got, again, (f"dw{l}", "two runs"))
