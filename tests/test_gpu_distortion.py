"""The distortion loss on the ragged training rays on the GPU (csrc/distortion.hip, include/pnr_distortion.h, raymarching.distortion_loss,
run_cuda's distortion=True, train_loss's lambda_distort) against the float64 statement of tests/distortion_reference.py."""
import types

import numpy as np
import pytest
import torch

from palettenerf_amd import raymarching
from palettenerf_amd._torch_glue import call, ptr
from tests import distortion_reference as dr
from tests import guarded

gpu = pytest.mark.gpu
T_THRESH = dr.T_THRESH

# The project's rule for a tolerance: 4 x a measured error of the formulation a user would write without the kernel.  E is the error of
# dr.per_op_fp32 (padded dense fp32 torch, autograd through cumprod / cumsum) against float64 on the main batch, as max abs error over max abs
# value, measured on an MI355X (profiles/distortion/README.md, "Tolerance"): dist 7.328e-06, grad_sigmas 3.530e-05.  In that run the kernel's own
# figures were 5.2e-07 and 1.2e-06.
TOL_DIST = 4 * 7.328e-06
TOL_GRAD = 4 * 3.530e-05
EXP_TOL = dict(rtol=2e-5, atol=2e-6)     # tests/test_gpu_ops.py:15, :364 -- what the 16-lane scan composite is held to against the sample-order oracle


def dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)       # (a copy: the cached batches are read-only)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), what


def rel_err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def forward_entry(sig, dl, rays, outs=None):
    """pnr_distortion_forward on device tensors -> (dist, w_sum, wm_sum); outs: the three arrays to write (default: fresh, NaN-filled)."""
    N = rays.shape[0]
    outs = outs or [torch.full((N,), float("nan"), device=sig.device) for _ in range(3)]
    call("pnr_distortion_forward", ptr(sig), ptr(dl), ptr(rays), sig.shape[0], N, T_THRESH, *(ptr(o) for o in outs))
    return outs


def backward_entry(gdist, sig, dl, rays, fwd, out=None):
    """pnr_distortion_backward -> grad_sigmas [M]; out: the array to write (default: fresh, NaN-filled: the entry writes every element)."""
    out = torch.full_like(sig, float("nan")) if out is None else out
    call("pnr_distortion_backward", ptr(gdist), ptr(sig), ptr(dl), ptr(rays), *(ptr(t) for t in fwd), sig.shape[0], rays.shape[0], T_THRESH, ptr(out))
    return out


def tensors(b, cuda):
    return dev(b["sig"], cuda), dev(b["dl"], cuda), dev(b["rays"], cuda), dev(b["gdist"], cuda)


def dead_ids(b):
    return [int(i) for i, o, c in b["rays"] if dr.ray_is_empty(int(o), int(c), b["M"])]


@gpu
@pytest.mark.parametrize("kind", ["main", "long_first", "one"])
def test_forward_against_float64(cuda, kind):
    b, t = dr.batch(kind), dr.truth(kind)
    dr.check_batch(b)                                   # no ray is left out of a comparison
    sig, dl, rays, _ = tensors(b, cuda)
    dist, w_sum, wm_sum = forward_entry(sig, dl, rays)
    print(f"{kind} dist: rel err {rel_err(host(dist), t['dist']):.3e} (allowed {TOL_DIST:.3e}), max {t['dist'].max():.3e}; "
          f"w_sum {rel_err(host(w_sum), t['w_sum']):.3e}, wm_sum {rel_err(host(wm_sum), t['wm_sum']):.3e} (max {t['wm_sum'].max():.3e})")
    assert np.abs(host(dist) - t["dist"]).max() <= TOL_DIST * np.abs(t["dist"]).max()
    np.testing.assert_allclose(host(w_sum), t["w_sum"], **EXP_TOL)
    span = max(float(t["wm_sum"].max()), 1.0)           # wm_sum = sum w m: the weights' tolerance at the scale of m
    np.testing.assert_allclose(host(wm_sum), t["wm_sum"], rtol=EXP_TOL["rtol"], atol=EXP_TOL["atol"] * span)
    for out in (dist, w_sum, wm_sum):
        assert bool((out[dev(np.array(dead_ids(b), np.int64), cuda)] == 0).all())          # empty and skipped rays: exactly 0
    # the operator is the entry's dist; w_sum is the training composite's weights_sum on the same batch
    same_bits(raymarching.distortion_loss(sig, dl, rays, T_THRESH), dist, "operator")
    ws, _, _ = raymarching.composite_rays_train(sig, torch.rand(b["M"], 3, device=cuda), dl, rays, T_THRESH)
    print(f"{kind} w_sum vs composite_rays_train's weights_sum: max abs diff {float((ws - w_sum).abs().max()):.3e}")
    np.testing.assert_allclose(host(w_sum), host(ws), **EXP_TOL)


@gpu
@pytest.mark.parametrize("kind", ["main", "long_first", "one"])
def test_backward_against_float64(cuda, kind):
    b, t = dr.batch(kind), dr.truth(kind)
    sig, dl, rays, gdist = tensors(b, cuda)
    grad = backward_entry(gdist, sig, dl, rays, forward_entry(sig, dl, rays))
    print(f"{kind} grad_sigmas: rel err {rel_err(host(grad), t['grad_sigmas']):.3e} (allowed {TOL_GRAD:.3e}), max {np.abs(t['grad_sigmas']).max():.3e}")
    assert np.abs(host(grad) - t["grad_sigmas"]).max() <= TOL_GRAD * np.abs(t["grad_sigmas"]).max()
    off = dev(~t["live"], cuda)                          # behind a stop, on skipped rays, owned by no ray
    assert (int(off.sum()) > 100 or kind == "one") and bool((grad[off] == 0).all())      # (the single ray runs its full length)
    assert bool((grad[dev(t["live"], cuda)] != 0).any())
    # through autograd
    s = sig.clone().requires_grad_(True)
    (raymarching.distortion_loss(s, dl, rays, T_THRESH) * gdist).sum().backward()
    same_bits(s.grad, grad, "autograd")
    assert dl.grad is None


@gpu
def test_two_launches_give_the_same_bits(cuda):
    sig, dl, rays, gdist = tensors(dr.batch("main"), cuda)
    a, b2 = forward_entry(sig, dl, rays), forward_entry(sig, dl, rays)
    for u, v in zip(a, b2):
        same_bits(u, v, "forward")
    same_bits(backward_entry(gdist, sig, dl, rays, a), backward_entry(gdist, sig, dl, rays, b2), "backward")


@gpu
def test_no_gradient_asked_and_empty_shapes(cuda):
    sig, dl, rays, gdist = tensors(dr.batch("main"), cuda)
    # autograd hands None to a backward whose output nobody differentiated (set_materialize_grads(False)): no launch, no gradients
    ctx = types.SimpleNamespace(_fwd_used_autocast=False, _dtype=torch.float32, saved_tensors=(), dims=[0, 0, T_THRESH])
    assert raymarching._distortion_loss.backward(ctx, None) == (None, None, None, None)
    s = sig.clone().requires_grad_(True)
    d = raymarching.distortion_loss(s, dl, rays, T_THRESH)
    assert d.requires_grad
    (s * 2).sum().backward()                             # the loss does not read d
    assert bool((s.grad == 2).all())
    with pytest.raises(RuntimeError):                    # no double backward
        s2 = sig.clone().requires_grad_(True)
        g, = torch.autograd.grad(raymarching.distortion_loss(s2, dl, rays, T_THRESH).sum(), s2, create_graph=True)
        g.sum().backward()
    # no rays; rays without samples
    none = raymarching.distortion_loss(sig, dl, rays[:0], T_THRESH)
    assert none.shape == (0,)
    s0 = torch.zeros(0, device=cuda, requires_grad=True)
    r0 = torch.tensor([[1, 0, 0], [0, 0, 5]], dtype=torch.int32, device=cuda)
    d0 = raymarching.distortion_loss(s0, torch.zeros(0, 2, device=cuda), r0, T_THRESH)
    assert d0.shape == (2,) and bool((d0 == 0).all())
    d0.sum().backward()
    assert s0.grad.shape == (0,)


@gpu
@pytest.mark.parametrize("align", [256, 4])
def test_guard_bands(cuda, align):
    """Both entries inside guard bands (tests/guarded.py): no byte written outside the outputs, no result that depends on a byte outside the inputs."""
    b = dr.batch("main")
    sig, dl, rays, gdist = tensors(b, cuda)
    plain = forward_entry(sig, dl, rays)
    plain_grad = backward_entry(gdist, sig, dl, rays, plain)
    N, M = b["N"], b["M"]
    ins = [guarded.inp(sig, align), guarded.inp(dl, align), guarded.inp(rays, align, around=(0, 0, 1)), guarded.inp(gdist, align)]
    (bs, gsig), (bd, gdl), (br, grays), (bg, ggd) = ins
    outs = [guarded.out((N,), torch.float32, cuda, align) for _ in range(3)]
    got = forward_entry(gsig, gdl, grays, [v for _, v in outs])
    fins = [guarded.inp(t, align) for t in got]           # the backward reads the forward's three arrays
    bgrad, vgrad = guarded.out((M,), torch.float32, cuda, align)
    backward_entry(ggd, gsig, gdl, grays, [v for _, v in fins], vgrad)
    torch.cuda.synchronize()
    for what, (buf, view) in zip(("sigmas", "deltas", "rays", "grad_dist", "dist", "w_sum", "wm_sum", "dist (read)", "w_sum (read)", "wm_sum (read)",
                                  "grad_sigmas"), ins + outs + fins + [(bgrad, vgrad)]):
        assert view.data_ptr() % 256 == align % 256
        assert guarded.untouched(buf, view), f"{what}: {guarded.last_report}"
    for u, v in zip(got, plain):
        same_bits(u, v, "forward inside bands")
    same_bits(vgrad, plain_grad, "backward inside bands")


# ------------------------------------------------------------------------------------------------ the model
def make_model(cuda):
    from palettenerf_amd import network, scene
    m = network.NeRFNetwork(bound=1, cuda_ray=True, min_near=0.05)
    scene.seed_field_(m, 0)
    m = m.to(cuda).train()
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid(bound=1)).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m


def rays256(cuda):
    from palettenerf_amd import scene
    H, W = 756, 1008
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3, 0.0, 1.5]
    ro, rd = scene.get_rays(torch.from_numpy(pose)[None], scene.intrinsics_from_fov(H, W, 0.9), H, W)
    g = torch.Generator().manual_seed(5)
    inds = torch.randint(0, H * W, [256], generator=g)
    return ro[:, inds].to(cuda), rd[:, inds].to(cuda), torch.rand(1, 256, 3, generator=g).to(cuda)


def model_step(m, cuda, render_kw, loss_kw, autocast=False):
    from palettenerf_amd.train_loss import train_loss
    ro, rd, gt = rays256(cuda)
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(3)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        r = m.render(ro, rd, staged=False, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=T_THRESH, **render_kw)
        loss, info = train_loss(r, gt, **loss_kw)
    loss.backward()
    return r, loss.detach(), info, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@gpu
def test_model_step(cuda, monkeypatch):
    """A 256-ray batch is below gridencoder.BINNED_MIN_ROWS, where the table gradient is a scatter of float atomics in arrival order; the steps
    take the binned (order-stable) table gradient instead, as tests/test_gpu_train_norm.py does."""
    from palettenerf_amd import gridencoder, trainset
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1)
    seen, op = [], raymarching.distortion_loss
    monkeypatch.setattr(raymarching, "distortion_loss", lambda *a: (seen.append(a), op(*a))[1])
    m = make_model(cuda)
    lam = 0.01
    r, loss, info, grads = model_step(m, cuda, dict(distortion=True), dict(lambda_distort=lam))
    assert len(seen) == 1
    sigmas, deltas, rays, thresh = seen[0]
    assert thresh == T_THRESH and sigmas.requires_grad and sigmas.shape[0] > 10_000 and rays.shape == (256, 3)
    d = r["distortion"]
    assert d.shape == r["weights_sum"].shape == (256,) and d.dtype == torch.float32 and d.requires_grad
    same_bits(d.detach(), op(sigmas.detach(), deltas, rays, thresh), "results['distortion'] is the op on what the composite read")
    assert float(d.detach().max()) > 0
    ws, _, _ = raymarching.composite_rays_train(sigmas.detach(), torch.zeros(sigmas.shape[0], 3, device=cuda), deltas, rays, thresh)
    same_bits(ws, r["weights_sum"].detach(), "the same sigmas / deltas / rays")
    # the loss: exactly lambda * mean more; loss_ray and loss_distort
    _, loss0, info0, grads0 = model_step(m, cuda, dict(distortion=True), dict())
    print(f"loss {float(loss0):.8e} + {lam} * {float(d.mean()):.6e} -> {float(loss):.8e}")
    same_bits(loss, loss0 + lam * d.detach().mean(), "loss")
    same_bits(info["loss_distort"], lam * d.detach().mean(), "loss_distort")
    same_bits(info["loss_ray"], info0["loss_ray"] + lam * d.detach().view(1, 256), "loss_ray")
    same_bits(info["terms"], info0["terms"], "terms")
    assert "loss_distort" not in info0
    # the term's own gradient reaches sigma_net and the table, and nothing behind sigma
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(3)
    ro, rd, _ = rays256(cuda)
    (lam * m.render(ro, rd, staged=False, perturb=True, force_all_rays=True, max_steps=1024, T_thresh=T_THRESH, distortion=True)["distortion"].mean()).backward()
    own = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    reached = {n for n, g in own.items() if float(g.abs().max()) > 0}
    print("the distortion term alone reaches", sorted(reached))
    assert {"encoder.embeddings", "sigma_net.0.weight", "sigma_net.1.weight"} <= reached and not any(n.startswith("color_net") for n in reached)
    assert all(bool(torch.isfinite(g).all()) for g in own.values())
    assert any(not torch.equal(grads[n], grads0[n]) for n in ("encoder.embeddings", "sigma_net.0.weight"))
    # a zero weight: the call without the argument, bit for bit, and no launch of the op
    del seen[:]
    ra, la, ia, ga = model_step(m, cuda, dict(), dict())
    rb, lb, ib, gb = model_step(m, cuda, dict(distortion=False), dict(lambda_distort=0.0))
    assert not seen and "distortion" not in ra and "distortion" not in rb
    same_bits(la, lb, "loss")
    same_bits(la, loss0, "loss without the term, with and without the render's flag")
    assert set(ga) == set(gb) == set(grads0) and set(ia) == set(ib)
    for n in ga:
        same_bits(ga[n], gb[n], n)
        same_bits(ga[n], grads0[n], n)                   # computing the map changes nothing that exists
    # trainset.train_step: the flag follows the weight
    batch = trainset.TrainBatch(ro, rd, rays256(cuda)[2], 1, None, None, None, None, None, 756, 1008)
    kw = dict(max_steps=1024, T_thresh=T_THRESH)
    torch.manual_seed(3)
    _, _, l1, ld1 = trainset.train_step(m, batch, kw, lambda_distort=lam)
    assert len(seen) == 1 and "loss_distort" in ld1 and float(ld1["loss_distort"]) > 0
    torch.manual_seed(3)
    _, _, l2, ld2 = trainset.train_step(m, batch, kw)
    assert len(seen) == 1 and "loss_distort" not in ld2
    same_bits(l1.detach(), l2.detach() + ld1["loss_distort"], "train_step")
    # inference ignores the flag
    m.eval()
    with torch.no_grad():
        out = m.render(ro, rd, staged=False, max_steps=1024, T_thresh=T_THRESH, distortion=True)
    assert "distortion" not in out and len(seen) == 1


@gpu
def test_model_step_under_fp16_autocast(cuda):
    m = make_model(cuda)
    r, loss, info, grads = model_step(m, cuda, dict(distortion=True), dict(lambda_distort=0.01), autocast=True)
    assert r["distortion"].dtype == torch.float32 and r["distortion"].shape == (256,)
    assert bool(torch.isfinite(r["distortion"]).all()) and float(r["distortion"].max()) > 0 and bool(torch.isfinite(loss))
    assert {"encoder.embeddings", "sigma_net.0.weight"} <= set(grads)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the operator itself under autocast, half sigmas: cast to fp32, fp32 out
    sig, dl, rays, _ = tensors(dr.batch("main"), cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = raymarching.distortion_loss(sig.half(), dl, rays, T_THRESH)
    same_bits(out, raymarching.distortion_loss(sig.half().float(), dl, rays, T_THRESH), "operator under autocast")
