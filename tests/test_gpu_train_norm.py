"""The NeRF stage's rgb_norm regulariser inside the training composite (pnr_composite_rays_train_norm_*, raymarching.composite_rays_train_norm,
NeRFRenderer.run_cuda with rays_gt, train_loss's lambda_sparse): against the plain composite (same bits), the CPU oracle chain
(spread_ray_to_sample -> norm -> composite of three equal channels), the reference's own kernels, and the per-op branch of the model."""
import functools

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import raymarching

gpu = pytest.mark.gpu

EXP_TOL = dict(rtol=2e-5, atol=2e-6)     # tests/test_gpu_ops.py:15 -- __expf (v_exp_f32) vs libm expf in the compositing kernels
GRAD_RGBS_TOL = dict(rtol=2e-5, atol=2e-6)      # tests/test_gpu_ops.py:359
GRAD_SIGMAS_TOL = dict(rtol=2e-4, atol=2e-5)    # tests/test_gpu_ops.py:360
T_THRESH = 1e-4
COOP_MIN_SAMPLES = 1 << 16               # kCoopMinSamples (csrc/composite.hip): from here on the 16-lanes-per-ray scan kernels
CYCLE = (0, 1, 15, 16, 17, 31, 32, 33)
MARGIN = 1e-3                            # no transmittance of the batch lies within this (relative) of T_thresh


def transmittance64(sig, dl, off, cnt):
    """Transmittance behind each of a ray's samples, float64."""
    s, d = sig[off:off + cnt].astype(np.float64), dl[off:off + cnt, 0].astype(np.float64)
    return np.cumprod(np.exp(-s * d))


@functools.lru_cache(maxsize=None)
def batch(kind):
    """small: 37 rays, M ~ 1e3 (the sample-order kernels); scan: 640 rays, M just above 65 536 (the scan kernels).  Ray lengths cycle through
    CYCLE, a few rays of 200-600 samples fill M; ray ids are a permutation; one ray overruns M; rays with one huge sigma stop on T_thresh at a
    chosen lane of a 16-sample group; every seventh ray id has its own colour as ground truth.  -> dict of numpy arrays (never modified)."""
    rng = np.random.default_rng({"small": 11, "scan": 12}[kind])
    N, n_long = (37, 2) if kind == "small" else (640, 160)
    counts = np.array([CYCLE[i % 8] for i in range(N - n_long)] + [0] * n_long)
    if kind == "small":
        counts[-n_long:] = (200, 250)
    else:
        long = rng.integers(200, 601, n_long)
        target = COOP_MIN_SAMPLES + 40 - int(counts.sum())
        while long.sum() != target:          # move single samples between the long rays until M is what it should be
            j = rng.integers(n_long)
            step = int(np.sign(target - long.sum()))
            if 200 <= long[j] + step <= 600:
                long[j] += step
        counts[-n_long:] = long
    order = rng.permutation(N)               # the long rays are not the last rows
    last17 = next(i for i in range(N) if counts[order[i]] == 17)
    order[[last17, N - 1]] = order[[N - 1, last17]]          # ... the last row is a 17-sample ray: the one that overruns M below
    counts = counts[order]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts.sum())
    ids = rng.permutation(N)
    rays = np.stack([ids, offs, counts], 1).astype(np.int32)
    sig = (rng.random(M) * 40).astype(np.float32)
    translucent = rng.random(N) < 0.5        # ... run their full length; the others stop on T_thresh somewhere after ~30 samples
    for n in np.nonzero(translucent)[0]:
        sig[offs[n]:offs[n] + counts[n]] *= 0.03
    rgb = rng.random((M, 3)).astype(np.float32)
    dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
    # forced stops: thin samples in front of sample `at`, which takes T far below the threshold -- at a group's first lane (at % 16 == 0), at its
    # last lane (15) and inside a group, in the first group and in later ones
    plan = [(32, 16), (32, 20), (33, 31), (33, 5)]
    plan += [(200, 15), (250, 48)] if kind == "small" else [(None, at) for at in (15, 16, 47, 48, 100, 191)]
    forced = {}
    for length, at in plan:
        n = next(n for n in range(N) if n not in forced and (counts[n] == length if length else counts[n] >= 200))
        forced[n] = at
        sig[offs[n]:offs[n] + at] = rng.random(at).astype(np.float32)
        sig[offs[n] + at] = np.float32(20.0 / dl[offs[n] + at, 0])
    # the ray whose rows would end behind M: dead, like an empty one.  (It is the last row and keeps its own rows, which no other ray reads:
    # kernel_spread_ray_to_sample writes an overrunning ray's rows up to M, raymarching.cu:874.)
    over = N - 1
    assert counts[over] == 17
    rays[over, 2] = 18
    # no boundary transmittance within MARGIN of T_thresh: redraw the sample's sigma where one is
    for n in range(N):
        if n == over or counts[n] == 0:
            continue
        for _ in range(100):
            T = transmittance64(sig, dl, offs[n], counts[n])
            bad = np.nonzero(np.abs(T / T_THRESH - 1) <= MARGIN)[0]
            if bad.size == 0:
                break
            sig[offs[n] + bad[0]] = np.float32(sig[offs[n] + bad[0]] * (1.0 + rng.random()))
    gt = rng.random((N, 3)).astype(np.float32)
    own = [int(rays[n, 0]) for n in range(N) if rays[n, 0] % 7 == 3 and n != over and counts[n] > 0]
    for n in range(N):
        if int(rays[n, 0]) in own:
            rgb[offs[n]:offs[n] + counts[n]] = gt[rays[n, 0]]      # the ray shows its own ground truth: every n_k is exactly 0
    # which rows take part (float64 restatement of the stop rule): the samples up to and including the first with T behind it below T_thresh
    live = np.zeros(M, bool)
    stops = {}
    for n in range(N):
        if n == over or counts[n] == 0:
            continue
        T = transmittance64(sig, dl, offs[n], counts[n])
        below = np.nonzero(T < T_THRESH)[0]
        last = int(below[0]) if below.size else int(counts[n]) - 1
        live[offs[n]:offs[n] + last + 1] = True
        if below.size:
            stops[n] = last
    g = dict(gws=rng.standard_normal(N).astype(np.float32), gimg=rng.standard_normal((N, 3)).astype(np.float32),
             gnorm=rng.standard_normal(N).astype(np.float32))
    out = dict(N=N, M=M, rays=rays, sig=sig, rgb=rgb, dl=dl, gt=gt, own=np.array(own), over=over, live=live, stops=stops, forced=forced, counts=counts,
               offs=offs, **g)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def norm32(gt_s, rgb):
    """n_k in fp32, channel order (torch's ((gt - rgb) ** 2).sum(-1) on a row of three)."""
    e = gt_s - rgb
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


@functools.lru_cache(maxsize=None)
def oracle_chain(kind):
    """The reference's chain on the CPU oracle, forward and backward -- computed once per batch."""
    b = batch(kind)
    gt_s = np.zeros((b["M"], 3), np.float32)
    oracle.spread_ray_to_sample(b["gt"], b["rays"], gt_s)
    n = norm32(gt_s, b["rgb"]).astype(np.float32)
    n3 = np.repeat(n[:, None], 3, 1)
    ws, dep, img = oracle.composite_rays_train_forward(b["sig"], b["rgb"], b["dl"], b["rays"], T_THRESH)
    nws, _, nimg = oracle.composite_rays_train_forward(b["sig"], n3, b["dl"], b["rays"], T_THRESH)
    gs1, gc1 = oracle.composite_rays_train_backward(b["gws"], b["gimg"], b["sig"], b["rgb"], b["dl"], b["rays"], ws, img, T_THRESH)
    third = np.repeat((b["gnorm"] / np.float32(3))[:, None], 3, 1).astype(np.float32)      # mean(dim=-1)'s backward
    gs2, gn3 = oracle.composite_rays_train_backward(np.zeros(b["N"], np.float32), third, b["sig"], n3, b["dl"], b["rays"], nws, nimg, T_THRESH)
    gn = gn3.sum(-1, dtype=np.float32)                                                       # repeat(1, 3)'s backward
    gc2 = gn[:, None] * np.float32(2) * (b["rgb"] - gt_s)                                    # ((gt - rgb) ** 2).sum(-1)'s backward
    return dict(ws=ws, dep=dep, img=img, norm=nimg[:, 0], grad_sigmas=gs1 + gs2, grad_rgbs=gc1 + gc2)


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)       # (a copy: the cached batches are read-only)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), what


def report(what, got, want):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max abs err {err.max():.3e}, max |want| {np.abs(want).max():.3e}")


@pytest.mark.parametrize("kind", ["small", "scan"])
def test_batch_construction(kind):
    """No device needed: the batches have what the GPU comparisons rely on."""
    b = batch(kind)
    assert (b["M"] >= COOP_MIN_SAMPLES) == (kind == "scan") and (kind == "small" or b["M"] < COOP_MIN_SAMPLES + 128)
    assert sorted(b["rays"][:, 0].tolist()) == list(range(b["N"])) and not np.array_equal(b["rays"][:, 0], np.arange(b["N"]))
    assert set(CYCLE) <= set(b["counts"].tolist()) and ((b["counts"] >= 200) & (b["counts"] <= 600)).sum() >= 2
    over = b["over"]
    assert b["rays"][over, 1] + b["rays"][over, 2] > b["M"]
    worst = np.inf
    for n in range(b["N"]):
        if n != over and b["counts"][n]:
            T = transmittance64(b["sig"], b["dl"], b["offs"][n], b["counts"][n])
            worst = min(worst, float(np.abs(T / T_THRESH - 1).min()))
    assert worst > MARGIN, worst
    lanes = {b["stops"][n] % 16 for n in b["forced"]}
    assert all(b["stops"][n] == at for n, at in b["forced"].items())            # the forced rays stop where they were told to
    assert {0, 15} <= lanes and lanes - {0, 15}                                  # a group's first lane, its last lane, and inside one
    assert all(b["counts"][n] > b["stops"][n] + 1 for n in b["forced"])          # ... with rows behind the stopping sample
    assert len(b["own"]) >= 3 and 0 < b["live"].sum() < b["M"]


def run_fused(b, cuda):
    ts, tc = dev(b["sig"], cuda).requires_grad_(True), dev(b["rgb"], cuda).requires_grad_(True)
    out = raymarching.composite_rays_train_norm(ts, tc, dev(b["dl"], cuda), dev(b["rays"], cuda), dev(b["gt"], cuda), T_THRESH)
    return ts, tc, out


@gpu
@pytest.mark.parametrize("kind", ["small", "scan"])
def test_forward_outputs(cuda, kind):
    b, o = batch(kind), oracle_chain(kind)
    with torch.no_grad():
        _, _, (ws, dep, img, norm) = run_fused(b, cuda)
        pws, pdep, pimg = raymarching.composite_rays_train(dev(b["sig"], cuda), dev(b["rgb"], cuda), dev(b["dl"], cuda), dev(b["rays"], cuda), T_THRESH)
    same_bits(ws, pws, "weights_sum")
    same_bits(dep, pdep, "depth")
    same_bits(img, pimg, "image")
    assert norm.shape == (b["N"],) and norm.dtype == torch.float32
    report(f"{kind} rgb_norm", host(norm), o["norm"])
    np.testing.assert_allclose(host(ws), o["ws"], **EXP_TOL)
    np.testing.assert_allclose(host(norm), o["norm"], **EXP_TOL)
    assert float(o["norm"].max()) > 0.05
    assert bool((norm[dev(b["own"], cuda).long()] == 0).all())                  # ground truth == the ray's colour: exactly zero
    dead = b["rays"][(b["counts"] == 0) | (np.arange(b["N"]) == b["over"]), 0]
    for t in (ws, dep, norm, img.abs().sum(-1)):
        assert bool((t[dev(dead, cuda).long()] == 0).all())


@gpu
@pytest.mark.parametrize("kind", ["small", "scan"])
def test_backward(cuda, kind):
    b, o = batch(kind), oracle_chain(kind)
    gws, gimg, gnorm = dev(b["gws"], cuda), dev(b["gimg"], cuda), dev(b["gnorm"], cuda)
    # nobody reads the norm: the plain operator's gradients, bit for bit
    ts, tc, (ws, dep, img, norm) = run_fused(b, cuda)
    ((ws * gws).sum() + (img * gimg).sum() + dep.sum()).backward()
    ps, pc = dev(b["sig"], cuda).requires_grad_(True), dev(b["rgb"], cuda).requires_grad_(True)
    pws, pdep, pimg = raymarching.composite_rays_train(ps, pc, dev(b["dl"], cuda), dev(b["rays"], cuda), T_THRESH)
    ((pws * gws).sum() + (pimg * gimg).sum() + pdep.sum()).backward()
    same_bits(ts.grad, ps.grad, "grad_sigmas without g_norm")
    same_bits(tc.grad, pc.grad, "grad_rgbs without g_norm")
    # with it: the oracle chain
    gt_t = dev(b["gt"], cuda).requires_grad_(True)
    ts, tc = dev(b["sig"], cuda).requires_grad_(True), dev(b["rgb"], cuda).requires_grad_(True)
    ws, dep, img, norm = raymarching.composite_rays_train_norm(ts, tc, dev(b["dl"], cuda), dev(b["rays"], cuda), gt_t, T_THRESH)
    ((ws * gws).sum() + (img * gimg).sum() + (norm * gnorm).sum() + dep.sum()).backward()
    assert gt_t.grad is None                                                     # rays_gt receives no gradient
    report(f"{kind} grad_rgbs", host(tc.grad), o["grad_rgbs"])
    report(f"{kind} grad_sigmas", host(ts.grad), o["grad_sigmas"])
    np.testing.assert_allclose(host(tc.grad), o["grad_rgbs"], **GRAD_RGBS_TOL)
    np.testing.assert_allclose(host(ts.grad), o["grad_sigmas"], **GRAD_SIGMAS_TOL)
    off = dev(~b["live"], cuda)                                                  # dead rays' rows, rows behind a stopping sample
    assert bool((ts.grad[off] == 0).all()) and bool((tc.grad[off] == 0).all())
    # only the norm is read
    ts2, tc2, (_, _, _, norm2) = run_fused(b, cuda)
    (norm2 * gnorm).sum().backward()
    assert bool((ts2.grad[off] == 0).all()) and float(tc2.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the model
def make_model(cuda):
    from palettenerf_amd import network, scene
    m = network.NeRFNetwork(bound=1, cuda_ray=True, min_near=0.05)
    scene.seed_field_(m, 0)
    m = m.to(cuda).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid(bound=1)).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m


@functools.lru_cache(maxsize=None)
def rays256():
    from palettenerf_amd import scene
    H, W = 756, 1008
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]
    ro, rd = scene.get_rays(torch.from_numpy(pose)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    g = torch.Generator().manual_seed(5)
    inds = torch.randint(0, H * W, [256], generator=g)
    return ro[:, inds].cuda(), rd[:, inds].cuda(), torch.rand(1, 256, 3, generator=g).cuda()


LAMBDA_SPARSE = 0.05     # main_nerf.py:67
# The project's rule for a gradient tolerance (tests/test_gpu_smooth.py): 4 x a measured disagreement, as max |g - g_ref| / max |g_ref| per parameter.
# The measured figure here is the disagreement of the per-op branch (fused_train_norm = False) of this very step with a float64 evaluation of the
# same step (profiles/sparse/grad_tolerance.py on an MI355X; profiles/sparse/README.md, "Gradient tolerance"), parameter by parameter.  In that
# run the fused branch differed from the per-op branch by 4.8e-8 ... 1.4e-7 of max |g|.
MEASURED_GRAD_ERR_VS_FLOAT64 = {"encoder.embeddings": 1.777e-3, "sigma_net.0.weight": 3.947e-4, "sigma_net.1.weight": 4.125e-6,
                                "color_net.0.weight": 1.416e-5, "color_net.1.weight": 3.179e-5, "color_net.2.weight": 8.241e-7}


def train_step(m, fused, perturb=True, autocast=False, seed=3, on_samples=None):
    from palettenerf_amd.train_loss import train_loss
    ro, rd, gt = rays256()
    m.fused_train_norm = fused
    for p in m.parameters():
        p.grad = None
    seen = {}

    def keep(module, args, out):      # the field's per-sample outputs: their gradients are what the composite's backward writes
        out[0].retain_grad(), out[1].retain_grad()
        seen.update(sigmas=out[0], rgbs=out[1])

    hook = m.register_forward_hook(keep)
    try:
        torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            r = m.run_cuda(ro, rd, rays_gt=gt, perturb=perturb, force_all_rays=True, max_steps=1024, T_thresh=T_THRESH)
            loss, info = train_loss(r, gt, lambda_sparse=LAMBDA_SPARSE)
        loss.backward()
    finally:
        hook.remove()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(r=r, loss=loss.detach(), info=info, grads=grads, weights_sum=r["weights_sum"].detach(), image_raw=r.raw.image_raw.detach(),
                depth_raw=r.raw.depth_raw.detach(), rgb_norm=r["rgb_norm"].detach(), grad_sigmas=seen["sigmas"].grad, grad_rgbs=seen["rgbs"].grad)


@gpu
def test_model_step_fused_against_the_per_op_branch(cuda, monkeypatch):
    """A 256-ray batch is below gridencoder.BINNED_MIN_ROWS, where the table gradient is a scatter of float atomics in arrival order; the step takes
    the binned (order-stable) table gradient instead, as tests/test_gpu_smooth.py:276-279 does."""
    from palettenerf_amd import gridencoder
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1)
    m = make_model(cuda)
    a, b = train_step(m, True), train_step(m, False)
    assert a["rgb_norm"].shape == (1, 256) and float(b["rgb_norm"].max()) > 0.01 and a["grad_sigmas"].shape[0] > 10_000
    same_bits(a["image_raw"], b["image_raw"], "image")
    same_bits(a["weights_sum"], b["weights_sum"], "weights_sum")
    same_bits(a["r"]["image"].detach(), b["r"]["image"].detach(), "blended image")
    report("model rgb_norm", host(a["rgb_norm"]), host(b["rgb_norm"]))
    np.testing.assert_allclose(host(a["rgb_norm"]), host(b["rgb_norm"]), **EXP_TOL)
    assert set(a["grads"]) == set(b["grads"]) and "encoder.embeddings" in a["grads"]
    worst = 0.0
    for n in b["grads"]:
        ref = float(b["grads"][n].abs().max())
        rel = float((a["grads"][n] - b["grads"][n]).abs().max()) / ref
        print(f"grad {n}: fused vs per-op rel diff {rel:.3e} (max |g| {ref:.3e})")
        worst = max(worst, rel)
    print(f"worst gradient rel diff {worst:.3e}; smallest allowance {4 * min(MEASURED_GRAD_ERR_VS_FLOAT64.values()):.3e}")
    assert set(b["grads"]) == set(MEASURED_GRAD_ERR_VS_FLOAT64)
    for n in b["grads"]:
        assert float((a["grads"][n] - b["grads"][n]).abs().max()) <= 4 * MEASURED_GRAD_ERR_VS_FLOAT64[n] * float(b["grads"][n].abs().max()), n
    # without a ground truth the flag is never looked at: the plain composite and a zero map
    ro, rd, _ = rays256()
    torch.manual_seed(3)
    r0 = m.run_cuda(ro, rd, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=T_THRESH)
    same_bits(r0["weights_sum"].detach(), a["weights_sum"], "weights_sum without rays_gt")
    assert float(r0["rgb_norm"].abs().max()) == 0 and r0["rgb_norm"].shape == (1, 256)


@gpu
def test_loss_takes_the_sparse_term(cuda):
    from palettenerf_amd.train_loss import TERM_NAMES, train_loss
    m = make_model(cuda)
    ro, rd, gt = rays256()
    torch.manual_seed(3)
    r = m.run_cuda(ro, rd, rays_gt=gt, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=T_THRESH)
    lam = LAMBDA_SPARSE
    loss, info = train_loss(r, gt, lambda_sparse=lam)
    with torch.no_grad():
        bracket = ((r["image"] - gt) ** 2).mean(-1) + lam * r["rgb_norm"]
        want = bracket.mean()
    print(f"loss {float(loss.detach()):.8e} torch {float(want):.8e}; loss_sparse {float(info['loss_sparse']):.4e}")
    assert abs(float(loss.detach()) - float(want)) <= 2e-6 * abs(float(want))                    # tests/test_train_loss.py:113
    # tests/test_train_loss.py:126's bound on loss_ray (rtol 3e-7) plus the one rounding of the sum that both sides add (2^-23)
    assert torch.allclose(info["loss_ray"], bracket, rtol=3e-7 + 2.0 ** -23, atol=1e-9)
    assert info["loss_ray"].shape == (1, 256) and not info["loss_ray"].requires_grad
    assert abs(float(info["loss_sparse"]) - lam * float(r["rgb_norm"].mean())) <= 1e-6 * float(info["loss_sparse"]) and float(info["loss_sparse"]) > 0
    assert info["terms"].shape == (len(TERM_NAMES),) == (10,)
    # a zero weight: today's result, bit for bit
    l0, i0 = train_loss(r, gt, lambda_sparse=0.0)
    l1, i1 = train_loss(r, gt)
    same_bits(l0.detach(), l1.detach(), "loss")
    same_bits(i0["loss_ray"], i1["loss_ray"], "loss_ray")
    same_bits(i0["terms"], i1["terms"], "terms")
    assert set(i0) == set(i1) and "loss_sparse" not in i0


@gpu
def test_autocast_gives_the_fp32_maps(cuda):
    m = make_model(cuda)
    a = train_step(m, True, autocast=False)
    b = train_step(m, True, autocast=True)
    for k in ("weights_sum", "image_raw", "depth_raw", "rgb_norm"):
        assert b[k].dtype == torch.float32, k
        print(f"autocast {k}: max abs diff to the fp32 run {float((a[k] - b[k]).abs().max()):.3e}")
    for k in ("weights_sum", "image_raw", "depth_raw", "rgb_norm"):
        same_bits(a[k], b[k], k)
    # the operator itself under autocast, half inputs: cast to fp32, fp32 out
    bt = batch("small")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = raymarching.composite_rays_train_norm(dev(bt["sig"], cuda).half(), dev(bt["rgb"], cuda).half(), dev(bt["dl"], cuda), dev(bt["rays"], cuda),
                                                    dev(bt["gt"], cuda).half(), T_THRESH)
    with torch.no_grad():
        want = raymarching.composite_rays_train_norm(dev(bt["sig"], cuda).half().float(), dev(bt["rgb"], cuda).half().float(), dev(bt["dl"], cuda),
                                                     dev(bt["rays"], cuda), dev(bt["gt"], cuda).half().float(), T_THRESH)
    for u, v in zip(out, want):
        same_bits(u, v, "operator under autocast")


# ------------------------------------------------------------------------------------------------ the reference's own kernels
@pytest.fixture(scope="module")
def ref_backend(cuda):
    import os
    from oracle import ref_build, ref_ops
    if not ref_ops.available():     # the rule of tests/test_gpu_reference_kernels.py: a missing build FAILS under -m gpu
        msg = "oracle/_ref/ref_*.so are not built (oracle/ref_build.py: build_hip needs the reference checkout at build time)"
        if os.environ.get("PNR_ALLOW_NO_REF") == "1":
            pytest.skip(msg + " -- PNR_ALLOW_NO_REF=1")
        pytest.fail(msg + "; set PNR_ALLOW_NO_REF=1 to run the GPU suite without the reference's kernels")
    return ref_build.load_hip("raymarching")


def add_reference_training_ops(rm, be):
    """composite_rays_train and spread_ray_to_sample of the reference's operator layer (raymarching/raymarching.py:238-291, 451-473) over its own
    compiled kernels, for the module oracle.ref_ops.swapped_in() installs (which carries the inference operators and the training march only)."""
    class _CompositeTrain(torch.autograd.Function):
        @staticmethod
        def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh):
            sigmas, rgbs = sigmas.contiguous(), rgbs.contiguous()
            M, N = sigmas.shape[0], rays.shape[0]
            ws, depth, image = torch.empty(N, device=sigmas.device), torch.empty(N, device=sigmas.device), torch.empty(N, 3, device=sigmas.device)
            be.composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, ws, depth, image)
            ctx.save_for_backward(sigmas, rgbs, deltas, rays, ws, depth, image)
            ctx.dims = [M, N, T_thresh]
            return ws, depth, image

        @staticmethod
        def backward(ctx, grad_ws, grad_depth, grad_image):
            sigmas, rgbs, deltas, rays, ws, depth, image = ctx.saved_tensors
            M, N, T_thresh = ctx.dims
            gs, gc = torch.zeros_like(sigmas), torch.zeros_like(rgbs)
            be.composite_rays_train_backward(grad_ws.contiguous(), grad_image.contiguous(), sigmas, rgbs, deltas, rays, ws, image, M, N, T_thresh, gs, gc)
            return gs, gc, None, None, None

    def spread_ray_to_sample(inp, rays, output):
        inp = inp.contiguous()
        be.spread_ray_to_sample(inp, rays, output.shape[0], inp.shape[0], inp.shape[-1], output)
        return tuple()

    rm.composite_rays_train = lambda s, c, d, r, T=1e-4: _CompositeTrain.apply(s, c, d, r, T)
    rm.spread_ray_to_sample = spread_ray_to_sample


@gpu
def test_fused_branch_against_the_reference_kernels(cuda, ref_backend):
    """The per-op branch over the reference's compiled march, spread_ray_to_sample and composite_rays_train (and backward) against the fused branch:
    same model, rays and seed.  The reference's march hands out sample rows in atomics order, so per-sample gradients are compared ray by ray."""
    from oracle import ref_ops
    from palettenerf_amd import renderer
    m = make_model(cuda)

    def step(fused):
        rm = renderer.raymarching
        march, seen = rm.march_rays_train, {}
        rm.march_rays_train = lambda *a, **k: (lambda out: (seen.update(rays=out[3]), out)[1])(march(*a, **k))
        try:
            out = train_step(m, fused, perturb=False)
        finally:
            rm.march_rays_train = march
        out["rays"] = seen["rays"]
        return out

    ours = step(True)
    with ref_ops.swapped_in():
        add_reference_training_ops(renderer.raymarching, ref_backend)
        assert renderer.raymarching._backend is ref_backend
        theirs = step(False)
    assert renderer.raymarching is raymarching
    for k, tol in (("weights_sum", EXP_TOL), ("image_raw", EXP_TOL), ("rgb_norm", EXP_TOL)):
        report(f"reference kernels {k}", host(ours[k]), host(theirs[k]))
        np.testing.assert_allclose(host(ours[k]), host(theirs[k]), err_msg=k, **tol)
    assert float(theirs["rgb_norm"].max()) > 0.01

    def by_ray(o):      # sample rows in (ray id, position on the ray) order
        rays = o["rays"][torch.argsort(o["rays"][:, 0].long())]
        counts = rays[:, 2].long()
        starts = torch.cumsum(counts, 0) - counts
        within = torch.arange(int(counts.sum()), device=cuda) - torch.repeat_interleave(starts, counts)
        return torch.repeat_interleave(rays[:, 1].long(), counts) + within, counts

    ia, ca = by_ray(ours)
    ib, cb = by_ray(theirs)
    assert torch.equal(ca, cb) and int(ca.sum()) > 10_000
    for k, tol in (("grad_rgbs", GRAD_RGBS_TOL), ("grad_sigmas", GRAD_SIGMAS_TOL)):
        report(f"reference kernels {k}", host(ours[k][ia]), host(theirs[k][ib]))
        np.testing.assert_allclose(host(ours[k][ia]), host(theirs[k][ib]), err_msg=k, **tol)
    assert float(theirs["grad_sigmas"].abs().max()) > 0
