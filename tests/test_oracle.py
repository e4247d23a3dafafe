"""CPU suite: the oracle against the golden vectors and against independent NumPy/PyTorch
formulations of the same mathematics (no GPU, no reference tree needed)."""
import colorsys
import os

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import scene
from tests import grid_reference as gr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------------------------------ SH
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_sh_matches_reference_torch_encoder(deg):
    g = np.load(os.path.join(GOLDEN, "sh_torch.npz"))
    np.testing.assert_allclose(oracle.sh_encode_forward(g["x"], deg), g[f"y{deg}"], atol=1e-6, rtol=0)


def test_sh_matches_reference_cuda_polynomials_off_sphere():
    g = np.load(os.path.join(GOLDEN, "sh_cuda_expr.npz"))
    y, d = oracle.sh_encode_forward(g["points"].astype(np.float32), 8, True)
    d = d.reshape(-1, 3, 64)
    for got, want in ((y, g["y"]), (d[:, 0], g["dx"]), (d[:, 1], g["dy"]), (d[:, 2], g["dz"])):
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)


def test_sh_lower_degree_is_prefix_of_higher():
    x = np.random.default_rng(0).standard_normal((50, 3)).astype(np.float32)
    y8 = oracle.sh_encode_forward(x, 8)
    for deg in range(1, 8):
        np.testing.assert_array_equal(oracle.sh_encode_forward(x, deg), y8[:, :deg * deg])


def test_sh_backward_is_grad_dot_dydx():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((20, 3)).astype(np.float32)
    y, d = oracle.sh_encode_forward(x, 4, True)
    g = rng.standard_normal(y.shape).astype(np.float32)
    gi = oracle.sh_encode_backward(g, 4, d)
    want = np.einsum("bc,bdc->bd", g.astype(np.float64), d.reshape(20, 3, 16).astype(np.float64))
    np.testing.assert_allclose(gi, want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------ integer ops
def test_morton_known_answer_and_roundtrip():
    assert oracle.morton3D(np.array([[1, 2, 3]]))[0] == 53
    rng = np.random.default_rng(2)
    c = rng.integers(0, 128, size=(5000, 3)).astype(np.int32)
    idx = oracle.morton3D(c)
    np.testing.assert_array_equal(idx.astype(np.uint32), scene.morton3d_np(c[:, 0], c[:, 1], c[:, 2]))
    np.testing.assert_array_equal(oracle.morton3D_invert(idx), c)
    full = oracle.morton3D(np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3))
    assert sorted(full.tolist()) == list(range(16 ** 3))  # bijection on the 16^3 sub-cube


def test_morton_edge_cases():
    assert oracle.morton3D(np.zeros((0, 3), np.int32)).shape == (0,)
    assert oracle.morton3D(np.array([[127, 127, 127]]))[0] == 128 ** 3 - 1
    assert oracle.morton3D(np.array([[1023, 1023, 1023]]))[0] == 2 ** 30 - 1  # 10 bits per axis is the maximum


def test_packbits_matches_numpy_and_is_strict():
    rng = np.random.default_rng(3)
    g = rng.random((2, 4096)).astype(np.float32)
    g[0, :8] = 0.5
    bf = oracle.packbits(g, 0.5)
    np.testing.assert_array_equal(bf, scene.packbits_np(g, 0.5))
    assert bf[0] == 0  # strict '>'


# ------------------------------------------------------------------------------------------ near/far
def test_near_far_known_answers():
    aabb = [-1, -1, -1, 1, 1, 1]
    n, f = oracle.near_far_from_aabb([[0, 0, -3]], [[0, 0, 1]], aabb, 0.2)  # axis aligned: 1/dx = inf
    assert (n[0], f[0]) == (2.0, 4.0)
    n, f = oracle.near_far_from_aabb([[0, 5, -3]], [[0, 0, 1]], aabb, 0.2)  # miss
    assert n[0] == f[0] == np.finfo(np.float32).max
    n, f = oracle.near_far_from_aabb([[0, 0, 0]], [[0.6, 0.0, 0.8]], aabb, 0.2)  # inside the box: near clamps to min_near
    assert n[0] == np.float32(0.2) and abs(f[0] - 1.25) < 1e-6


def test_near_far_matches_vectorised_slab_test():
    rng = np.random.default_rng(4)
    o = rng.uniform(-3, 3, (4000, 3)).astype(np.float32)
    d = rng.standard_normal((4000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n, f = oracle.near_far_from_aabb(o, d, [-2, -2, -2, 2, 2, 2], 0.05)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = np.float32(1) / d
        t0, t1 = (np.float32(-2) - o) * rd, (np.float32(2) - o) * rd
    tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    hit = tn <= tf
    np.testing.assert_array_equal(n[~hit], np.finfo(np.float32).max)
    np.testing.assert_array_equal(f[hit], tf[hit])
    np.testing.assert_array_equal(n[hit], np.maximum(tn[hit], np.float32(0.05)))


# ------------------------------------------------------------------------------------------ HSV
def test_hsv_against_colorsys_and_roundtrip():
    rng = np.random.default_rng(5)
    rgb = rng.random((500, 3)).astype(np.float32)
    hsv = oracle.rgb_to_hsv(rgb)
    want = np.array([colorsys.rgb_to_hsv(*map(float, p)) for p in rgb]) * [360, 100, 100]
    np.testing.assert_allclose(hsv, want, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(oracle.hsv_to_rgb(hsv), rgb, atol=2e-6)
    np.testing.assert_allclose(oracle.rgb_to_hsv([[0.2, 0.5, 0.7]])[0], [204.0, 71.42857, 70.0], rtol=1e-6)
    np.testing.assert_array_equal(oracle.rgb_to_hsv([[0.25, 0.25, 0.25], [0, 0, 0]]), [[0, 0, 25], [0, 0, 0]])  # grey / black


# ------------------------------------------------------------------------------------------ compositing
def _rand_rays(rng, N, max_len, pad=3):
    counts = rng.integers(0, max_len, N)
    counts[0] = 0
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts.sum()) + pad
    rays = np.stack([rng.permutation(N), offs, counts], 1).astype(np.int32)
    sig = (rng.random(M) * 30).astype(np.float32)
    rgb = rng.random((M, 3)).astype(np.float32)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    return rays, sig, rgb, dl, M


def _torch_composite(sig, feat, dl, rays, N):
    """Independent formulation: alpha compositing by exclusive cumprod, no early termination."""
    out = torch.zeros(N, feat.shape[1], dtype=torch.float64)
    ws = torch.zeros(N, dtype=torch.float64)
    dep = torch.zeros(N, dtype=torch.float64)
    for idx, off, cnt in rays.tolist():
        if cnt == 0:
            continue
        s, d = sig[off:off + cnt], dl[off:off + cnt]
        alpha = 1 - torch.exp(-s * d[:, 0])
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1 - alpha[:-1]]), 0)
        w = alpha * T
        out[idx] = (w[:, None] * feat[off:off + cnt]).sum(0)
        ws[idx] = w.sum()
        dep[idx] = (w * torch.cumsum(d[:, 1], 0)).sum()
    return ws, dep, out


def test_composite_train_forward_backward_against_autograd():
    rng = np.random.default_rng(6)
    N = 40
    rays, sig, rgb, dl, M = _rand_rays(rng, N, 30)
    ws, dep, img = oracle.composite_rays_train_forward(sig, rgb, dl, rays, T_thresh=0.0)  # T<0 never true: no early stop
    ts = torch.tensor(sig, dtype=torch.float64, requires_grad=True)
    tc = torch.tensor(rgb, dtype=torch.float64, requires_grad=True)
    tws, tdep, timg = _torch_composite(ts, tc, torch.tensor(dl, dtype=torch.float64), rays, N)
    np.testing.assert_allclose(ws, tws.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dep, tdep.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(img, timg.detach().numpy(), rtol=1e-5, atol=1e-6)
    gws = rng.standard_normal(N).astype(np.float32)
    gimg = rng.standard_normal((N, 3)).astype(np.float32)
    (tws * torch.tensor(gws, dtype=torch.float64)).sum().add((timg * torch.tensor(gimg, dtype=torch.float64)).sum()).backward()
    gs, gc = oracle.composite_rays_train_backward(gws, gimg, sig, rgb, dl, rays, ws, img, T_thresh=0.0)
    np.testing.assert_allclose(gc, tc.grad.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(gs, ts.grad.numpy(), rtol=2e-3, atol=2e-5)


def test_composite_quirks():
    rng = np.random.default_rng(7)
    N = 8
    rays, sig, rgb, dl, M = _rand_rays(rng, N, 10, pad=0)
    # quirk 1: '>' for rgb, '>=' for flex: a ray ending exactly at M is composited by the former, zeroed by the latter
    last = int(np.argmax(rays[:, 1] + rays[:, 2]))
    assert rays[last, 1] + rays[last, 2] == M
    ws, dep, img = oracle.composite_rays_train_forward(sig, rgb, dl, rays)
    flex = oracle.composite_rays_flex_train_forward(sig, rgb, dl, rays)
    assert ws[rays[last, 0]] > 0 and np.all(flex[rays[last, 0]] == 0)
    other = [i for i in range(N) if i != last and rays[i, 2] > 0]
    np.testing.assert_array_equal(flex[rays[other, 0]], img[rays[other, 0]])
    # quirk 2: flex backward gives the terminating sample no gradient
    sig2 = np.full(6, 1e4, np.float32)
    dl2 = np.full((6, 2), 0.01, np.float32)
    r2 = np.array([[0, 0, 5]], np.int32)
    gi = oracle.composite_rays_flex_train_backward(np.ones((1, 2), np.float32), sig2, np.ones((6, 2), np.float32), dl2, r2)
    assert np.all(gi == 0)  # first sample already drives T below the threshold -> break before any write
    out = oracle.composite_rays_flex_train_forward(sig2, np.ones((6, 2), np.float32), dl2, r2)
    assert np.all(out > 0.99)  # ... while the forward did accumulate it
    # quirk 3: training depth integrates deltas[:,1] from 0
    ws, dep, img = oracle.composite_rays_train_forward(np.array([1e4, 0], np.float32), np.ones((2, 3), np.float32),
                                                       np.array([[0.01, 0.7], [0, 0]], np.float32), np.array([[0, 0, 1]], np.int32))
    assert abs(dep[0] - 0.7) < 1e-6


def test_composite_inference_chunking_matches_training_recurrence():
    """Feeding one ray's samples to composite_rays in chunks accumulates the same weights as the
    training kernel (T = 1 - ws vs the running product differ only by rounding)."""
    rng = np.random.default_rng(8)
    cnt = 37
    sig = (rng.random(cnt) * 20).astype(np.float32)
    rgb = rng.random((cnt, 3)).astype(np.float32)
    dl = np.stack([np.full(cnt, 0.01), np.full(cnt, 0.01)], 1).astype(np.float32)
    ws_t, dep_t, img_t = oracle.composite_rays_train_forward(sig, rgb, dl, np.array([[0, 0, cnt]], np.int32), T_thresh=1e-4)
    alive = np.array([0], np.int32)
    rays_t = np.array([0.0], np.float32)
    ws, dep, img = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros((1, 3), np.float32)
    pos, n_step = 0, 4
    while alive[0] >= 0 and pos < cnt:
        k = min(n_step, cnt - pos)
        s = np.zeros(n_step, np.float32); c = np.zeros((n_step, 3), np.float32); d = np.zeros((n_step, 2), np.float32)
        s[:k], c[:k], d[:k] = sig[pos:pos + k], rgb[pos:pos + k], dl[pos:pos + k]
        oracle.composite_rays(1, n_step, alive, rays_t, s, c, d, ws, dep, img, T_thresh=1e-4)
        pos += k
    np.testing.assert_allclose(ws, ws_t, rtol=1e-5)
    np.testing.assert_allclose(img, img_t, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dep, dep_t, rtol=1e-5, atol=1e-6)
    assert alive[0] == -1  # ran out of samples (delta == 0 sentinel) or T fell below the threshold


def test_composite_rays_flex_reads_but_never_writes_state():
    rng = np.random.default_rng(9)
    n_alive, n_step, nc = 5, 3, 20
    alive = np.arange(n_alive, dtype=np.int32)
    rays_t = rng.random(n_alive).astype(np.float32)
    ws = (rng.random(n_alive) * 0.5).astype(np.float32)
    sig = (rng.random(n_alive * n_step) * 10).astype(np.float32)
    inp = rng.random((n_alive * n_step, nc)).astype(np.float32)
    dl = np.full((n_alive * n_step, 2), 0.02, np.float32)
    out = np.zeros((n_alive, nc), np.float32)
    a0, t0, w0 = alive.copy(), rays_t.copy(), ws.copy()
    oracle.composite_rays_flex(n_alive, n_step, nc, alive, rays_t, sig, inp, dl, ws, out)
    assert (alive == a0).all() and (rays_t == t0).all() and (ws == w0).all() and out.any()
    # and it equals composite_rays on the same weights, channel by channel
    d, img = np.zeros(n_alive, np.float32), np.zeros((n_alive, 3), np.float32)
    oracle.composite_rays(n_alive, n_step, alive, rays_t, sig, inp[:, :3].copy(), dl, ws, d, img)
    np.testing.assert_array_equal(img, out[:, :3])


# ------------------------------------------------------------------------------------------ hash grid
def _torch_grid(x, emb, offsets, pls, H, L, C):
    """Independent vectorised formulation (float64 interpolation, integer maths in int64)."""
    primes = [1, 2654435761, 805459861]
    scales, ress = oracle.grid_level_params(L, pls, H)  # host-precomputed per-level constants (inputs of the kernels)
    outs = []
    for l in range(L):
        scale, res = scales[l], int(ress[l])
        assert res == int(np.ceil(scale)) + 1 and abs(float(scale) - (H * float(pls) ** l - 1)) < 1e-3 * (float(scale) + 1)
        T = int(offsets[l + 1] - offsets[l])
        # single-rounded x*scale+0.5 (== fmaf): the product of two binary32 numbers is exact in binary64
        pos = (x.detach().numpy() * np.float64(scale) + 0.5).astype(np.float32)
        pg = np.floor(pos).astype(np.int64)
        fr32 = torch.from_numpy((pos - pg.astype(np.float32)).astype(np.float64))  # the fp32 fractional part the kernel interpolates with
        fr = x * float(scale) + 0.5 - torch.from_numpy(pg).double()
        fr = fr + (fr32 - fr.detach())  # value of fr32, derivative d fr / d x = scale
        acc = 0
        for corner in range(8):
            bits = [(corner >> d) & 1 for d in range(3)]
            c = pg + np.array(bits)
            w = torch.ones(x.shape[0], dtype=torch.float64)
            for d in range(3):
                w = w * (fr[:, d] if bits[d] else 1 - fr[:, d])
            stride, idx, hashed = 1, np.zeros(len(c), np.int64), False
            for d in range(3):
                if stride <= T:
                    idx += c[:, d] * stride
                    stride *= res + 1
            if stride > T:
                idx = np.zeros(len(c), np.int64)
                for d in range(3):
                    idx ^= (c[:, d] * primes[d]) & 0xFFFFFFFF
            idx = idx % T + int(offsets[l])
            acc = acc + w[:, None] * emb[torch.from_numpy(idx)]
        outs.append(acc)
    return torch.cat(outs, 1)


@pytest.mark.parametrize("cfg", [dict(L=16, H=16, log2T=19, desired=4096), dict(L=6, H=4, log2T=8, desired=None)])
def test_grid_encode_forward_backward_against_independent_torch(cfg):
    rng = np.random.default_rng(10)
    L, H, C = cfg["L"], cfg["H"], 2
    pls = np.exp2(np.log2(cfg["desired"] / H) / (L - 1)) if cfg["desired"] else 2.0
    offsets = oracle.grid_offsets(3, L, pls, H, cfg["log2T"])
    emb = (rng.random((int(offsets[-1]), C)) - 0.5).astype(np.float32)
    x = rng.random((300, 3)).astype(np.float32)
    out, dydx = oracle.grid_encode_forward(x, emb, offsets, pls, H, calc_grad_inputs=True)
    te = torch.tensor(emb, dtype=torch.float64, requires_grad=True)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = _torch_grid(tx, te, offsets, pls, H, L, C)
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-4, atol=3e-6)
    g = rng.standard_normal(out.shape).astype(np.float32)
    (ref * torch.tensor(g, dtype=torch.float64)).sum().backward()
    gg, gi = oracle.grid_encode_backward(g, x, emb.shape, offsets, pls, H, dy_dx=dydx)
    np.testing.assert_allclose(gg, te.grad.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(gi, tx.grad.numpy(), rtol=2e-3, atol=2e-2 * np.abs(tx.grad.numpy()).max())


def test_grid_encode_level_sizes_match_survey():
    offsets = oracle.grid_offsets(3, 16, np.exp2(np.log2(4096 / 16) / 15), 16, 19)
    sizes = np.diff(offsets)
    assert sizes[:5].tolist() == [4920, 15632, 42880, 125000, 373248] and (sizes[5:] == 524288).all() and offsets[-1] == 6328848


def test_grid_encode_out_of_range_inputs_give_zeros():
    offsets = oracle.grid_offsets(3, 4, 2.0, 4, 8)
    emb = np.ones((int(offsets[-1]), 2), np.float32)
    x = np.array([[0.5, 0.5, 1.0001], [-1e-6, 0.2, 0.2], [0.0, 1.0, 0.5]], np.float32)
    out, dydx = oracle.grid_encode_forward(x, emb, offsets, 2.0, 4, calc_grad_inputs=True)
    assert np.all(out[:2] == 0) and np.all(dydx[:2] == 0) and np.all(out[2] > 0)  # boundaries 0 and 1 are inside
    gg = oracle.grid_encode_backward(np.ones_like(out), x, emb.shape, offsets, 2.0, 4)
    assert gg.sum() > 0 and np.isclose(gg.sum(), 8.0)  # only the in-range sample scatters: 4 levels * 2 channels * sum(w)=1


def test_grid_encode_gradcheck_recipe_of_reference_test():
    """testing/test_hashgrid_grad.py: L=4, C=2, H=4, T=2^8 (offsets without the /8 rounding there), one point,
    eps=1e-2, atol=1e-3, rtol=0.01 -- central differences on the embeddings."""
    rng = np.random.default_rng(11)
    offsets = np.array([0, 125, 381, 637, 893], np.int32)  # min(2^8, (4*2^i+1)^3)
    emb = (rng.standard_normal((893, 2)) * 0.1).astype(np.float32)
    x = rng.random((1, 3)).astype(np.float32)
    out = oracle.grid_encode_forward(x, emb, offsets, 2, 4)
    g = np.ones_like(out)
    gg = oracle.grid_encode_backward(g, x, emb.shape, offsets, 2, 4)
    touched = np.argwhere(gg != 0)
    assert 0 < len(touched) <= 4 * 8 * 2
    for r, c in touched[:: max(1, len(touched) // 12)]:
        e = emb.copy(); e[r, c] += 1e-2
        up = oracle.grid_encode_forward(x, e, offsets, 2, 4).sum()
        e[r, c] -= 2e-2
        dn = oracle.grid_encode_forward(x, e, offsets, 2, 4).sum()
        assert abs((up - dn) / 2e-2 - gg[r, c]) < 1e-3 + 0.01 * abs(gg[r, c])


def test_grid_encode_half_table_accumulates_in_half():
    rng = np.random.default_rng(12)
    offsets = oracle.grid_offsets(3, 8, 1.6, 16, 14)
    emb = (rng.random((int(offsets[-1]), 2)) - 0.5).astype(np.float16)
    x = rng.random((200, 3)).astype(np.float32)
    h = oracle.grid_encode_forward(x, emb, offsets, 1.6, 16)
    f = oracle.grid_encode_forward(x, emb.astype(np.float32), offsets, 1.6, 16)
    assert h.dtype == np.float16
    np.testing.assert_allclose(h.astype(np.float32), f, atol=2e-3)
    assert np.abs(h.astype(np.float32) - f).max() > 0  # the half accumulator is visibly not the fp32 one


@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
def test_grid_oracle_every_variant_against_float64(D, C):
    """The oracle is what the GPU kernels are compared with, so it is itself compared with the float64 statement of tests/grid_reference.py for every
    D x C x gridtype x align_corners (plus tiny tables for D <= 2 and hand-made odd level sizes), on ray-ordered and uniform inputs: fp32 forward, dy_dx,
    table gradient, input gradient, and the half-table forward -- each inside the bound that module derives for the precision of the number format."""
    L = gr.L
    fails = []

    def check(what, got, want, bound):
        r = gr.error_ratio(got, want, bound)
        if not r <= 1.0:
            fails.append(f"{what}: error / bound = {r}")

    cases = gr.variant_cases(D)
    assert {(g, a) for _, _, g, a in cases} == {(0, False), (0, True), (1, False), (1, True)}
    for ci, (name, offsets, gridtype, ac) in enumerate(cases):
        emb, g999 = gr.variant_tables(D, C, ci)
        emb16 = emb.astype(np.float16)
        for xname, x in gr.variant_inputs(D).items():
            B, g = x.shape[0], g999[: x.shape[0]]
            ref = gr.variant_geometry(D, ci, xname)
            tag = f"D{D} C{C} {name} {xname}"
            out, dydx = oracle.grid_encode_forward(x, emb, offsets, gr.PLS, gr.H, calc_grad_inputs=True, gridtype=gridtype, align_corners=ac)
            gg, gi = oracle.grid_encode_backward(g, x, emb.shape, offsets, gr.PLS, gr.H, gridtype=gridtype, align_corners=ac, dy_dx=dydx)
            want, mag = ref.forward(emb)
            check(tag + " forward", out.reshape(B, L, C), want, gr.forward_bound(D, mag))
            dy, dmag = ref.dy_dx(emb)
            check(tag + " dy_dx", dydx.reshape(B, L, D, C), dy, gr.dy_dx_bound(D, dmag))
            gt, gmag, n = ref.table_grad(g)
            check(tag + " table gradient", gg, gt, gr.table_grad_bound(D, gmag, n))
            assert n.sum() == ref.inr.sum() * L * 2 ** D and not gg[n == 0].any()
            wi, imag = ref.input_grad(g, dy, dmag)
            check(tag + " input gradient", gi, wi, gr.input_grad_bound(D, L, C, imag))
            assert not out[~ref.inr].any() and not dydx[~ref.inr].any() and not gi[~ref.inr].any()
            half = oracle.grid_encode_forward(x, emb16, offsets, gr.PLS, gr.H, gridtype=gridtype, align_corners=ac)
            want16, mag16 = ref.forward(emb16)
            check(tag + " half forward", half.reshape(B, L, C), want16, gr.forward_bound(D, mag16, gr.U16))
    assert not fails, "\n".join(fails)


def test_grid_reference_runs_of_equal_rows_cover_the_segmented_sum_cases():
    """What the GPU matrix relies on in its ray-ordered input: on the coarse levels consecutive samples share table rows in runs of many lengths, runs
    cross wave (64) and block (256) edges, an out-of-range sample sits inside a run, and the last wave is ragged."""
    for D in (1, 3, 5):
        ref = gr.variant_geometry(D, 0, "rays")
        assert ref.B == 999 and ref.B % 64 != 0 and (~ref.inr).sum() == 4 and not ref.inr[[100, 200, 500, 600]].any() and ref.inr[[400, 401]].all()
        rows = np.where(ref.inr, ref.rows[0, 0], -1)          # level 0, corner 0: what the kernel compares between neighbouring lanes
        edges = np.flatnonzero(np.diff(rows) != 0) + 1
        lengths = np.diff(np.concatenate([[0], edges, [999]]))
        assert lengths.max() >= 10 and len(set(lengths.tolist())) >= 5 and (lengths == 1).any()
        assert any(ref.rows[l, 0, 99] == ref.rows[l, 0, 101] for l in range(5))   # the far-outside sample 100 breaks a run in two
        for edge in (64, 256, 512):                           # some level has a run that continues across this wave / block edge
            assert any(ref.rows[l, 0, edge - 1] == ref.rows[l, 0, edge] for l in range(5))
        fine = np.where(ref.inr, ref.rows[4, 0], -1)
        assert (np.diff(fine) != 0).mean() > 0.3              # level 4 (still the combining kernel): mostly short runs
    uni = gr.variant_geometry(3, 0, "uniform")
    assert uni.B == 257 and (np.diff(uni.rows[4, 0]) != 0).mean() > 0.95


@pytest.mark.parametrize("D,C,case,xname", [(3, 2, 0, "rays"), (2, 4, 5, "uniform"), (5, 1, 4, "rays")])
def test_grid_reference_sparse_table_gradient_is_the_dense_one(D, C, case, xname):
    """table_grad_sparse (what the GPU test of the shipped 6-million-row geometry uses) against the dense table_grad on variant cases -- a dense level,
    a tiny hashed table, odd level sizes: the same rows, and the same float64 bits on them."""
    ref = gr.variant_geometry(D, case, xname)
    g = gr.variant_tables(D, C, case)[1][: ref.B]
    gt, mag, n = ref.table_grad(g)
    touched, s_gt, s_mag, s_n = ref.table_grad_sparse(g)
    assert np.array_equal(touched, np.flatnonzero(n)) and len(touched) > 0
    assert np.array_equal(s_n, n[touched]) and np.array_equal(s_gt, gt[touched]) and np.array_equal(s_mag, mag[touched])
    for dense, assembled in zip((gt, mag, n), ref.table_grad_from_sparse(g)):
        assert dense.dtype == assembled.dtype and np.array_equal(dense, assembled)


# ------------------------------------------------------------------------------------------ march
@pytest.fixture(scope="module")
def s0():
    grid = scene.brick_density_grid()
    return grid, oracle.packbits(grid, 0.5)


def _rays(H, W):
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(H, W), H, W)
    return ro[0].numpy(), rd[0].numpy()


def test_scene_s0_calibration(s0):
    grid, bf = s0
    assert int((grid[0] > 0).sum()) == 444528 and int((grid[1] > 0).sum()) == 55566
    np.testing.assert_array_equal(bf, scene.packbits_np(grid, 0.5))


@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
def test_march_train_samples_are_in_occupied_cells_and_rows_are_prefix_sums(s0, dt_gamma):
    grid, bf = s0
    ro, rd = _rays(24, 24)
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.2)
    cnt = np.zeros(2, np.int32)
    xyzs, dirs, deltas, rays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, nears, fars, cnt, align=128, force_all_rays=True, dt_gamma=dt_gamma)
    m = int(cnt[0])
    assert cnt[1] == 576 and xyzs.shape[0] % 128 == 0 and xyzs.shape[0] >= m and m > 0
    np.testing.assert_array_equal(rays[:, 0], np.arange(576))
    np.testing.assert_array_equal(rays[:, 1], np.concatenate([[0], np.cumsum(rays[:, 2])[:-1]]))
    assert rays[:, 2].sum() == m and np.all(deltas[m:] == 0) and np.all(deltas[:m, 0] > 0)
    # every emitted sample sits in an occupied cell of the cascade the kernel picked for it
    p = xyzs[:m]
    mx = np.abs(p).max(1)
    _, e = np.frexp(mx)
    lvl_dt = np.maximum(np.frexp(deltas[:m, 0] * 128 * 0.5)[1], 0)
    lvl = np.clip(np.maximum(e, lvl_dt), 0, 1)
    mb = np.minimum(np.exp2(lvl), 2.0)[:, None]
    cell = np.clip((0.5 * (p / mb + 1) * 128), 0, 127).astype(np.uint32)
    index = lvl.astype(np.uint32) * 128 ** 3 + scene.morton3d_np(cell[:, 0], cell[:, 1], cell[:, 2])
    assert np.all((bf[index // 8] >> (index % 8)) & 1)
    if dt_gamma == 0:
        assert np.all(deltas[:m, 0] == np.float32(2 * np.float32(1.7320508075688772) / 1024))


def test_march_inference_single_chunk_equals_training_march(s0):
    grid, bf = s0
    ro, rd = _rays(20, 20)
    N = ro.shape[0]
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.2)
    cnt = np.zeros(2, np.int32)
    xt, dtt, dlt, rays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, nears, fars, cnt, force_all_rays=True)
    n_step = int(rays[:, 2].max())
    x, d, dl = oracle.march_rays(N, n_step, np.arange(N, dtype=np.int32), nears.copy(), ro, rd, 2.0, bf, 2, 128, nears, fars, align=128)
    assert x.shape[0] == N * n_step + (128 - (N * n_step) % 128)  # always pads, even when aligned (quirk 4)
    for n in range(0, N, 7):
        off, c = rays[n, 1], rays[n, 2]
        np.testing.assert_array_equal(x[n * n_step:n * n_step + c], xt[off:off + c])
        np.testing.assert_array_equal(dl[n * n_step:n * n_step + c], dlt[off:off + c])
        assert np.all(dl[n * n_step + c:(n + 1) * n_step] == 0)


def test_march_train_drops_rays_that_overflow_M(s0):
    grid, bf = s0
    ro, rd = _rays(16, 16)
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.2)
    cnt = np.zeros(2, np.int32)
    xyzs, dirs, deltas, rays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, nears, fars, cnt, mean_count=1000, align=128)
    M = xyzs.shape[0]
    assert M == 1024 and cnt[0] > M  # counter keeps counting past M
    over = rays[:, 1] + rays[:, 2] > M
    assert over.any()
    first_over = int(np.argmax(over))
    assert np.all(deltas[rays[first_over, 1]:M] == 0)  # nothing written for the overflowing ray
    ws, dep, img = oracle.composite_rays_train_forward(np.ones(M, np.float32), np.ones((M, 3), np.float32), deltas, rays)
    assert np.all(ws[rays[over, 0]] == 0)


# ------------------------------------------------------------------------------------------ independent formulation of the march
def _fma32(a, b, c):
    """Correctly rounded float32 fma in NumPy: the product of two float32 is exact in float64; the float64 sum is corrected with its exact
    rounding error (TwoSum) when it lands on a float32 rounding midpoint, so that rounding to float32 happens once."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.uint64) if s.ndim else np.array(s).view(np.uint64)
    mid = (bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    nudge = mid & (err != 0) & np.isfinite(s)
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def _numpy_march(ro, rd, bf, nears, fars, bound, C, H, dt_gamma, max_steps):
    """All rays advance together, one probe per loop turn (masks instead of per-thread control flow); array arithmetic in float32 with the
    canonical contractions spelled out through _fma32.  Written from raymarching.cu:340-403 alone: shares no code with oracle/pnr_oracle.c
    or the HIP kernels.  Returns per-ray counts and the emitted samples (ray, x, y, z, dt, t_after) in per-ray order."""
    f32 = np.float32
    o, d = ro.astype(f32), rd.astype(f32)
    with np.errstate(divide="ignore"):
        rdir = (f32(1) / d).astype(f32)
    sgn = np.copysign(f32(1), d).astype(f32)
    N = o.shape[0]
    sqrt3 = f32(1.7320508075688772)
    dt_min = f32(f32(2) * sqrt3 / f32(max_steps))
    dt_max = f32(f32(f32(2) * sqrt3 * f32(1 << (C - 1))) / f32(H))
    rH = f32(1) / f32(H)
    clamp = lambda x, lo, hi: np.fmin(f32(hi), np.fmax(f32(lo), x)).astype(f32)   # fminf / fmaxf drop NaNs exactly like np.fmin / np.fmax
    t = nears.astype(f32).copy()
    t = _fma32(clamp(t * f32(dt_gamma), dt_min, dt_max), np.zeros(N, f32), t)   # perturb with noise 0 (kept: it turns -0 / NaN cases the same way)
    far = fars.astype(f32)
    count = np.zeros(N, np.int64)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            act = np.nonzero((t < far) & (count < max_steps))[0]
            if act.size == 0:
                break
            ta = t[act]
            p = clamp(_fma32(ta[:, None], d[act], o[act]), -bound, bound)
            dt = clamp(ta * f32(dt_gamma), dt_min, dt_max)
            e_pos = np.frexp(np.abs(p).max(1))[1]
            e_dt = np.frexp((dt * f32(H)).astype(f32) * f32(0.5))[1]
            level = np.clip(np.maximum(e_pos, e_dt), 0, C - 1).astype(np.int64)
            mip_bound = np.fmin(np.ldexp(f32(1), level).astype(f32), f32(bound)).astype(f32)
            mip_rbound = (f32(1) / mip_bound).astype(f32)
            cell_f = (0.5 * _fma32(p, mip_rbound[:, None], f32(1)).astype(np.float64) * float(H)).astype(f32)     # double intermediate, then float
            cell = clamp(cell_f, 0.0, float(H - 1)).astype(np.int64)                                                # truncation
            index = level * H ** 3 + scene.morton3d_np(cell[:, 0], cell[:, 1], cell[:, 2]).astype(np.int64)
            occ = ((bf[index // 8] >> (index % 8)) & 1).astype(bool)
            hit = act[occ]
            t_after = (ta[occ] + dt[occ]).astype(f32)
            out.append(np.column_stack([hit.astype(np.float64), p[occ].astype(np.float64), dt[occ].astype(np.float64), t_after.astype(np.float64)]))
            count[hit] += 1
            t[hit] = t_after
            miss = ~occ
            if miss.any():
                am = act[miss]
                inner = _fma32(f32(0.5), sgn[am], (cell[miss].astype(f32) + f32(0.5)).astype(f32))
                inner = (inner * rH).astype(f32)
                plane = _fma32(_fma32(inner, f32(2), f32(-1)), mip_bound[miss][:, None], -p[miss])
                txyz = (plane * rdir[am]).astype(f32)
                tt = (ta[miss] + np.fmax(f32(0), np.fmin(txyz[:, 0], np.fmin(txyz[:, 1], txyz[:, 2])))).astype(f32)
                tc = ta[miss].copy()
                go = np.ones(tc.shape, bool)
                while go.any():   # do { t += clamp(t * dt_gamma, dt_min, dt_max); } while (t < tt);
                    tc[go] = (tc[go] + clamp(tc[go] * f32(dt_gamma), dt_min, dt_max)).astype(f32)
                    go &= tc < tt
                t[am] = tc
    rows = np.concatenate(out) if out else np.zeros((0, 6))
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    return count, rows


@pytest.mark.parametrize("dt_gamma,min_near,HW", [(0.0, 0.2, (40, 30)), (1.0 / 128, 0.02, (32, 24)), (1.0 / 32, 0.2, (20, 20))])
def test_march_against_an_independent_numpy_formulation(s0, dt_gamma, min_near, HW):
    """The oracle's march (and with it the HIP kernels, which equal the oracle bit for bit) against a second, array-style statement of
    raymarching.cu:340-403 that shares no code with it: per-ray counts, positions, step sizes and parameters must be the same bits."""
    grid, bf = s0
    ro, rd = _rays(*HW)
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], min_near)
    cnt = np.zeros(2, np.int32)
    xyzs, dirs, deltas, rays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, nears, fars, cnt, force_all_rays=True, dt_gamma=dt_gamma)
    count, rows = _numpy_march(ro, rd, bf, nears, fars, 2.0, 2, 128, dt_gamma, 1024)
    m = int(cnt[0])
    assert m > 2000
    np.testing.assert_array_equal(count, rays[:, 2])                              # per-ray counts: bit-exact
    assert rows.shape[0] == m
    np.testing.assert_array_equal(rows[:, 1:4].astype(np.float32), xyzs[:m])      # sample positions
    np.testing.assert_array_equal(rows[:, 4].astype(np.float32), deltas[:m, 0])   # step sizes
    np.testing.assert_array_equal(rows[:, 0].astype(np.int64), np.repeat(np.arange(ro.shape[0]), rays[:, 2]))


def test_fma32_helper_is_a_correctly_rounded_fma():
    rng = np.random.default_rng(9)
    a = rng.standard_normal(200000).astype(np.float32)
    b = rng.standard_normal(200000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2.0 ** -12)   # heavy cancellation
    want = np.array([np.float32(np.longdouble(x) * np.longdouble(y) + np.longdouble(z)) for x, y, z in zip(a[:20000], b[:20000], c[:20000])])
    np.testing.assert_array_equal(_fma32(a[:20000], b[:20000], c[:20000]), want)
    # a constructed double-rounding trap: a*b + c lies just above a float32 midpoint, the float64 sum lands exactly on it
    a1, b1 = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)          # product = 1 + 2^-11 + 2^-24 exactly
    c1 = np.float32(2.0 ** -60)
    assert _fma32(a1, b1, c1) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)     # round up (true value is above the midpoint), not to even


# ------------------------------------------------------------------------------------------ build variants of the oracle
def test_oracle_openmp_variant_is_bit_identical(s0):
    from oracle import orc
    grid, bf = s0
    ro, rd = _rays(48, 48)
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.2)
    N = ro.shape[0]
    alive = np.arange(N, dtype=np.int32)
    rng = np.random.default_rng(3)
    pls = float(np.exp2(np.log2(4096 / 16) / 15))
    offsets = oracle.grid_offsets(3, 16, pls, 16, 19)
    emb = (rng.random((int(offsets[-1]), 2)) - 0.5).astype(np.float32)

    def run():
        x, d, dl = oracle.march_rays(N, 4, alive, nears.copy(), ro, rd, 2.0, bf, 2, 128, nears, fars, align=128)
        enc = oracle.grid_encode_forward((x + 2) / 4, emb, offsets, pls, 16)
        sh = oracle.sh_encode_forward(d, 4)
        ws, dep, img, al, rt = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32), alive.copy(), nears.copy()
        oracle.composite_rays(N, 4, al, rt, np.abs(enc[:, 0]) * 50, np.abs(enc[:, 1:4]), dl, ws, dep, img, 1e-4)
        return x, dl, enc, sh, ws, dep, img, al, rt

    a = run()
    prev = orc.use_variant("omp")
    try:
        orc.set_threads(4)
        b = run()
    finally:
        orc.use_variant(prev)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_oracle_without_contraction_reproduces_the_reference_measured_counts(s0):
    """SURVEY.md Appendix B ran the reference's own kernel_march_rays_train as host code (g++ -ffp-contract=off, i.e. NO fused multiply-adds)
    on scene S0 at 400 x 400: 88 725 rays with samples, at most 508 per ray, 15 750 694 samples.  The no-FMA build of the oracle is that
    arithmetic: hitting rays and the per-ray maximum are equal; the total agrees to 3 samples in 15.75 M (the survey's ray generator is not
    recorded: three fp32 ray generators tried here -- float64 + one rounding, the reference's torch get_rays, the device kernel -- differ in
    last bits of the directions and move the total by +-5).  The canonical build (explicit fmaf where nvcc contracts) differs from the
    no-FMA build by 7 samples at this size: that is the whole effect of the contraction choice."""
    from oracle import orc
    grid, bf = s0
    ro, rd = _rays(400, 400)
    nears, fars = oracle.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.2)
    res = {}
    for variant in ("nofma", ""):
        prev = orc.use_variant(variant)
        try:
            cnt = np.zeros(2, np.int32)
            rays = oracle.march_rays_train(ro, rd, 2.0, bf, 2, 128, nears, fars, cnt, mean_count=1, align=128)[3]   # M tiny: counting pass only
        finally:
            orc.use_variant(prev)
        res[variant] = (int(cnt[0]), int((rays[:, 2] > 0).sum()), int(rays[:, 2].max()))
    assert res["nofma"][1:] == (88725, 508) and res[""][1:] == (88725, 508)          # Appendix B, exact
    assert abs(res["nofma"][0] - 15750694) <= 8                                       # Appendix B's total, to the ray generator's last bits
    assert res["nofma"][0] == 15750697 and res[""][0] == 15750690                     # pinned: the two builds on this repo's deterministic rays


# ------------------------------------------------------------------------------------------ RGB histogram: the reference's own compiled code
def test_rgb_histogram_against_the_reference_build(golden_dir):
    """tests/golden/hist.npz was produced by palette/src/bindings.cpp:40-91 itself (compiled unmodified, oracle/ref_build.py); when the built
    module is present it is also called directly.  Integer bin indices and double accumulation in input order: bit-exact."""
    g = np.load(os.path.join(golden_dir, "hist.npz"))
    rgb, w = g["colors_rgb"], g["weights"]
    for bpc in (1, 2, 3, 5):
        bw, bc = oracle.compute_RGB_histogram(rgb, w, bpc)
        np.testing.assert_array_equal(bw, g[f"bin_weights_{bpc}"])
        np.testing.assert_array_equal(bc, g[f"bin_centers_{bpc}"])
    from oracle import ref_build
    if ref_build.available():
        mod = ref_build.load()
        rng = np.random.default_rng(8)
        rgb2 = rng.uniform(-0.2, 1.2, (20001, 3)).astype(np.float32)
        w2 = rng.uniform(0, 1, 20001).astype(np.float32)
        for bpc in (1, 4, 6):
            rbw, rbc = mod.compute_RGB_histogram(rgb2.flatten(), w2.flatten(), bpc)
            bw, bc = oracle.compute_RGB_histogram(rgb2, w2, bpc)
            np.testing.assert_array_equal(bw, np.asarray(rbw))
            np.testing.assert_array_equal(bc, np.asarray(rbc))


# ------------------------------------------------------------------------------------------ occupancy maintenance
def _occupancy_fixture():
    g = np.load(os.path.join(GOLDEN, "occupancy.npz"))
    return g, int(g["G"]), 2


def test_occupancy_full_sweep_against_the_reference_method():
    """tests/golden/occupancy.npz holds what the reference's own NeRFRenderer.update_extra_state (nerf/renderer.py:467-561, imported
    unmodified, CPU) drew, queried and left behind.  The oracle, fed the same random numbers, must produce the same points; fed the
    reference's sigmas, the same density grid, mean and bitfield."""
    g, G, C = _occupancy_fixture()
    noise = g["full_noise_u8"].astype(np.float32) / 256
    xyz, cells, p4 = oracle.occupancy_points(C, G, float(g["bound"]), noise)
    assert np.array_equal(cells, np.arange(C * G ** 3, dtype=np.int32))
    got, ref = xyz.reshape(C, G ** 3, 3)[:, ::16], g["full_points_every16"]
    # the reference ran on the CPU, where torch divides by (G - 1); on a GPU -- the canonical form, restated by the oracle -- torch multiplies
    # by the fp32 reciprocal: at most one ulp apart
    assert np.abs(got - ref).max() <= 2.4e-7 * float(g["bound"])
    grid = np.zeros((C, G ** 3), np.float32)
    cand = (g["full_sigma"] * np.float32(g["density_scale"])).reshape(-1)
    bits, mean, thresh = oracle.occupancy_commit(grid, p4, cand, 0.95, 1e9)
    assert np.array_equal(grid, g["full_grid"])
    assert abs(mean - float(g["full_mean"])) <= 1e-6 * mean and thresh == mean      # torch's fp32 tree sum vs the exact (fp64) mean
    near = np.abs(grid - mean) <= 1e-6 * mean
    diff = np.unpackbits(bits ^ g["full_bitfield"], bitorder="little").reshape(C, -1).astype(bool)
    assert not (diff & ~near).any() and diff.sum() <= near.sum()


def test_occupancy_partial_sweep_against_the_reference_method():
    """The partial sweep (iter_density >= 16): uniform cells + cells drawn from the occupied list, with repeats.  The reference keeps the
    LAST candidate of a repeated cell on one CPU thread (an unspecified one on a GPU); the oracle keeps the largest.  So: every cell of the
    reference's grid is one of the oracle's candidates for it, and where a cell was drawn once the two agree exactly."""
    g, G, C = _occupancy_fixture()
    n = G ** 3 // 4
    before = g["part_before"].copy()
    xyz, cells, p4 = oracle.occupancy_points(C, G, float(g["bound"]), g["part_noise_u8"].astype(np.float32) / 256, coords=g["part_coords_u8"].astype(np.int32),
                                             occ_rand=g["part_occ_rand"], density_grid=before, n_partial=n)
    assert np.abs(xyz.reshape(C, 2 * n, 3)[:, ::16] - g["part_points_every16"]).max() <= 2.4e-7 * float(g["bound"])
    assert (cells >= 0).all() and not np.isin(cells.reshape(C, 2 * n)[:, n:], np.arange(64)).any()      # the 64 retired cells (density -1) are never drawn from the occupied list ...
    grid = before.copy()
    cand = (g["part_sigma"] * np.float32(g["density_scale"])).reshape(-1)
    decay, dth = float(g["part_decay"]), float(g["part_density_thresh"])
    bits, mean, thresh = oracle.occupancy_commit(grid, p4, cand, decay, dth)
    assert thresh == np.float32(dth) and mean > dth
    ref = g["part_grid"]
    assert np.array_equal(grid[0, :64], before[0, :64]) and (grid[0, :64] == -1).all()     # ... and never updated
    counts = np.bincount(cells, minlength=C * G ** 3).reshape(C, -1)
    once = counts <= 1
    assert np.array_equal(grid[once], ref[once])
    assert (grid >= ref).all()
    order = np.argsort(cells, kind="stable")
    sc, sv = cells[order], np.maximum(before.reshape(-1)[cells[order]] * np.float32(decay), cand[order])
    flat_ref = ref.reshape(-1)
    hit = np.zeros(C * G ** 3, bool)
    np.logical_or.at(hit, sc, sv == flat_ref[sc])
    drawn = np.unique(cells)
    drawn = drawn[before.reshape(-1)[drawn] >= 0]      # (retired cells may be drawn by the uniform half; they keep their -1)
    assert hit[drawn].all()          # the reference's value of every drawn cell is one of its candidates
    assert np.array_equal(np.unpackbits(bits, bitorder="little").reshape(C, -1).astype(bool), grid > thresh)


@pytest.mark.parametrize("key,filt", [("mark_grid", False), ("mark_grid_filter_close", True)])
def test_mark_untrained_grid_against_the_reference_method(key, filt):
    g, G, C = _occupancy_fixture()
    grid = np.zeros((C, G ** 3), np.float32)
    n = oracle.mark_untrained_grid(g["mark_poses"], g["mark_intrinsics"], grid, float(g["bound"]), 0.2, filt)
    ref = np.unpackbits(g[key])[:C * G ** 3].reshape(C, -1).astype(bool)
    assert n == int(ref.sum()) and np.array_equal(grid < 0, ref)
    assert 0 < n < C * G ** 3


# ------------------------------------------------------------------------------------------ round 4: the reference's OWN operator wrappers over the oracle
def test_reference_operator_wrappers_over_the_native_stand_ins_equal_the_restated_facades(golden_dir):
    """tests/golden/gen_golden.py drove the reference's own gridencoder/grid.py, shencoder/sphere_harmonics.py and the composite Functions of
    raymarching/raymarching.py (their `_backend` = oracle/native_facade.py) through wrapper_outputs() and recorded the exact results
    (tests/golden/wrapper_digests.json).  oracle/facade.py -- the restatement bench.py's cpu_baseline and the host-logic tests still use -- must give
    the very same bytes: GridEncoder construction, forward with the bound map, table gradient, the half-table forward, SHEncoder, the training
    composites forward + backward, the in-place inference composites."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(golden_dir, "gen_golden.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    from oracle.facade import make_oracle_modules
    rm, ge, sh, _ = make_oracle_modules()
    got = gg.wrapper_outputs(rm, ge, sh, gg.oracle_half_encode)
    assert float(np.abs(got["composite_flex_infer"]).sum()) > 0
    want = json.load(open(os.path.join(golden_dir, "wrapper_digests.json")))
    mine = gg.digests(got)
    assert sorted(mine) == sorted(want)
    assert [k for k in want if mine[k] != want[k]] == []


def test_pure_torch_encoders_of_the_cpu_baseline_against_the_oracle():
    """oracle/torch_encoders.py (bench.py's configs[0] leg: the "pure-PyTorch" CPU path) against the C oracle."""
    from oracle.torch_encoders import TorchGridEncoder, TorchSHEncoder
    torch.manual_seed(3)
    g = TorchGridEncoder(num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096)
    with torch.no_grad():
        g.embeddings.uniform_(-0.5, 0.5)
    x = torch.rand(4000, 3) * 4 - 2
    x[:3] = torch.tensor([[2.0, 2.0, 2.0], [-2.0, -2.0, -2.0], [2.0000005, 0.0, 0.0]])
    with torch.no_grad():
        out = g(x, bound=2).numpy()
    want = oracle.grid_encode_forward(((x + 2) / 4).numpy(), g.embeddings.detach().numpy(), g.offsets.numpy(), g.per_level_scale, 16)
    np.testing.assert_allclose(out, want, rtol=0, atol=2e-7)       # same cells and weights; torch's a*b+c is not contracted where the oracle's fmaf is
    assert (out[2] == 0).all()                                      # outside [0, 1]: zeros
    d = torch.randn(1000, 3)
    d = d / d.norm(dim=1, keepdim=True)
    for deg in (1, 2, 3, 4):
        np.testing.assert_allclose(TorchSHEncoder(degree=deg)(d).numpy(), oracle.sh_encode_forward(d.numpy(), deg), rtol=0, atol=1e-6)


def test_oracle_against_the_reference_wrapper_fixture_fp32_and_autocast(golden_dir):
    """grid_autocast.npz (the reference's GridEncoder over the native stand-ins, fp32 and with the autocast flag on): the oracle's NumPy front
    end -- offsets, level scales, the [L,B,C] permute restated -- reproduces both outputs from the seed alone."""
    fx = np.load(os.path.join(golden_dir, "grid_autocast.npz"))
    offs = oracle.grid_offsets(3, 16, float(fx["per_level_scale"]), 16, 19)
    np.testing.assert_array_equal(offs, fx["offsets"])
    g = torch.Generator().manual_seed(int(fx["seed"]))
    emb = (torch.rand(int(offs[-1]), 2, generator=g) - 0.5).numpy()
    x01 = ((torch.from_numpy(fx["x"]) + 2.0) / 4.0).numpy()
    np.testing.assert_array_equal(oracle.grid_encode_forward(x01, emb, offs, float(fx["per_level_scale"]), 16), fx["y32"])
    np.testing.assert_array_equal(oracle.grid_encode_forward(x01, emb.astype(np.float16), offs, float(fx["per_level_scale"]), 16).view(np.uint16), fx["y16_bits"])
