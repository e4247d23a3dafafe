"""tests/distortion_reference.py on the CPU: the float64 statement against a recorded run of the reference's own EffDistLoss
(tests/golden/distortion_effdist.npz, written by tests/golden/gen_distortion_golden.py), the prefix form and the closed-form gradient the
kernel uses against the pairwise statement and autograd, the per-op fp32 formulation against the statement, and the conditions of the batch
the GPU tests run on.  No device."""
import os

import numpy as np
import torch

from tests import distortion_reference as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distortion_effdist.npz")


def test_statement_against_the_recorded_effdistloss():
    g = np.load(GOLDEN)
    w, m, iv = g["w"], g["m"], g["interval"]
    B, K = w.shape
    assert (B, K) == (8, 24) and w.dtype == np.float64
    total, grads, closed = 0.0, [], []
    for r in range(B):
        wt = torch.tensor(w[r], requires_grad=True)
        value = dr.pairwise64(wt, torch.tensor(m[r]), torch.tensor(iv[r]))
        value.backward()
        total += float(value.detach())
        grads.append(wt.grad.numpy())
        dist, v = dr.prefix_form64(w[r], m[r], iv[r])
        assert abs(dist - float(value.detach())) <= 1e-12
        closed.append(v)
    print(f"loss: statement {total / B:.17g} recorded {float(g['loss']):.17g}")
    assert abs(total - B * float(g["loss"])) <= 1e-12                      # EffDistLoss divides by n_rays
    assert np.abs(np.stack(grads) - B * g["grad_w"]).max() <= 1e-12
    assert np.abs(np.stack(closed) - B * g["grad_w"]).max() <= 1e-12


def test_batch_conditions():
    b = dr.batch("main")
    N, M, rays = b["N"], b["M"], b["rays"]
    assert N == 48 and 2800 <= M <= 3200
    assert set(rays[:, 2].tolist()) == set(dr.STEPS)
    assert sorted(rays[:, 0].tolist()) == list(range(N)) and not np.array_equal(rays[:, 0], np.arange(N))
    over = b["over"]
    assert rays[over, 1] + rays[over, 2] > M and rays[over, 1] < M
    assert sum(dr.ray_is_empty(int(o), int(c), M) and c > 0 for _, o, c in rays) == 1
    worst = dr.check_batch(b)
    print(f"closest transmittance to T_thresh: factor 1 +- {worst:.3e}")
    t = dr.truth("main")
    stops = {n: t["stops"][n] for n in b["forced"]}
    assert stops == b["forced"] and sorted(stops.values()) == [4, 31, 32]            # opaque by sample 5; lane 15 of a group; lane 0 of the next
    assert all(rays[n, 2] > k + 1 for n, k in stops.items())                          # ... with rows behind the stopping sample
    # absolute t reaches 80
    t_max = max(float(np.cumsum(b["dl"][o:o + c, 1].astype(np.float64)).max()) for _, o, c in rays if c and o + c <= M)
    assert t_max >= 80.0, t_max
    # a stretch that no ray owns, inside [0, M)
    owned = np.zeros(M, bool)
    for n, (_, o, c) in enumerate(rays):
        if n != over:
            assert not owned[o:o + c].any()                                           # rays do not share samples
            owned[o:o + c] = True
    lo, hi = b["gap"]
    assert 0 < lo < hi < M and hi - lo >= 100 and not owned[lo:hi].any() and owned[lo - 1] and owned[hi]
    assert not t["live"][~owned].any() and 0 < t["live"].sum() < owned.sum()          # some owned samples lie behind a stop
    # a ray that runs its full 600 samples and one that stops inside them
    long_stops = sorted(t["stops"][n] for n in range(N) if rays[n, 2] == 600)
    assert long_stops[1] == 599 and 16 < long_stops[0] < 599
    assert float(t["dist"].max()) > 1e-3 and float(np.abs(t["grad_sigmas"]).max()) > 1e-4
    dead = [int(i) for i, o, c in rays if dr.ray_is_empty(int(o), int(c), M)]
    assert len(dead) == 5 and not t["dist"][dead].any()
    # the variants
    lf = dr.batch("long_first")
    assert lf["rays"][0, 2] == 600 and sorted(map(tuple, lf["rays"].tolist())) == sorted(map(tuple, rays.tolist()))
    tl = dr.truth("long_first")
    assert np.array_equal(tl["dist"], t["dist"]) and np.array_equal(tl["grad_sigmas"], t["grad_sigmas"])
    one = dr.batch("one")
    assert one["N"] == 1 and one["M"] == 33 and dr.check_batch(one) > dr.MARGIN


def test_prefix_form_and_closed_gradient_against_the_statement():
    b, t = dr.batch("main"), dr.truth("main")
    worst_v, worst_g, scale = 0.0, 0.0, float(np.abs(t["grad_sigmas"]).max())
    for n in range(b["N"]):
        idx, off, cnt = (int(v) for v in b["rays"][n])
        if dr.ray_is_empty(off, cnt, b["M"]):
            continue
        w, m, d, _ = dr.ray_weights64(b["sig"], b["dl"], off, cnt)
        dist, _ = dr.prefix_form64(w, m, d)
        rel, _ = dr.prefix_form64(w, m - m[0], d)                                     # the value does not depend on where m starts
        worst_v = max(worst_v, abs(dist - t["dist"][idx]), abs(rel - t["dist"][idx]))
        assert abs((w * (m - m[0])).sum() - t["wm_sum"][idx]) <= 1e-13 and abs(w.sum() - t["w_sum"][idx]) <= 1e-14
        g = b["gdist"][idx].astype(np.float64) * dr.grad_sigma_closed64(b["sig"], b["dl"], off, cnt)
        worst_g = max(worst_g, float(np.abs(g - t["grad_sigmas"][off:off + g.shape[0]]).max()))
        assert not t["grad_sigmas"][off + g.shape[0]:off + cnt].any()
    print(f"prefix form vs pairwise: value {worst_v:.3e} (max {t['dist'].max():.3e}), gradient {worst_g:.3e} (max {scale:.3e})")
    assert worst_v <= 1e-12 * max(1.0, float(t["dist"].max()))                        # m up to 86: 2e-14 per product, a few hundred terms
    assert worst_g <= 1e-12 * scale


def test_per_op_fp32_formulation_is_the_same_quantity():
    b, t = dr.batch("main"), dr.truth("main")
    s = torch.from_numpy(b["sig"]).requires_grad_(True)
    dist = dr.per_op_fp32(s, torch.from_numpy(b["dl"]), torch.from_numpy(b["rays"]))
    (dist * torch.from_numpy(b["gdist"])).sum().backward()
    e_dist = np.abs(dist.detach().numpy() - t["dist"]).max() / np.abs(t["dist"]).max()
    e_grad = np.abs(s.grad.numpy() - t["grad_sigmas"]).max() / np.abs(t["grad_sigmas"]).max()
    print(f"per-op fp32 on the CPU vs float64: dist {e_dist:.3e}, grad_sigmas {e_grad:.3e}")
    assert dist.dtype == torch.float32 and e_dist < 1e-3 and e_grad < 1e-3              # the same quantity; its fp32 error is measured on the GPU
    assert not s.grad.numpy()[~t["live"]].any()
