"""The distortion loss of the ragged training rays (include/pnr_distortion.h, raymarching.distortion_loss), stated in float64: what
csrc/distortion.hip is tested against (tests/test_distortion_host.py, tests/test_gpu_distortion.py).

For one ray with the samples and the stop rule of composite_rays_train (raymarching.cu:537-570): alpha_k = 1 - exp(-sigma_k d_k), w_k = alpha_k T_k,
T_{k+1} = T_k (1 - alpha_k); the sample that brings T below T_thresh still counts, the ones behind it have w = 0; num_steps == 0 or
offset + num_steps > M is an empty ray.  With m_k the running sum of deltas[:,1] and d_k = deltas[k,0]:

    dist = sum_{i,j} w_i w_j |m_i - m_j| + (1/3) sum_k d_k w_k^2

The VALUE here is that pairwise sum, not the prefix form the kernel uses, and the GRADIENT is torch autograd in float64 through the
sample-order loop: neither shares the kernel's algebra.  `prefix_form64` is the kernel's algebra in float64 (the reference's EffDistLoss per
ray, and the closed-form gradient), held against the pairwise statement in tests/test_distortion_host.py.

`per_op_fp32` is what a user without the kernel would write: the rays padded to a dense [N, max_steps] fp32 matrix, torch.cumprod for the
transmittance, torch.cumsum for m (absolute, as `depth` sums it) and for the prefix sums, autograd for the gradient.  Its error against
float64 on the test batch is the yardstick E of the kernel's tolerance (profiles/distortion/README.md)."""
import functools

import numpy as np
import torch

T_THRESH = 1e-4
MARGIN = 1e-3            # no transmittance of a batch lies within this (relative) of T_thresh: fp32 and float64 stop at the same sample
STEPS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 100, 600)


# ------------------------------------------------------------------------------------------------ float64
def ray_is_empty(off, cnt, M):
    return cnt == 0 or off + cnt > M


def ray_weights64(sig, dl, off, cnt, T_thresh=T_THRESH):
    """-> (w [K], m [K], d [K], T [K]: the transmittance BEHIND each sample) of the K samples that count, float64 numpy, sample order."""
    w, m, d, Ts = [], [], [], []
    T, t = 1.0, 0.0
    for k in range(off, off + cnt):
        alpha = 1.0 - np.exp(-np.float64(sig[k]) * np.float64(dl[k, 0]))
        t += np.float64(dl[k, 1])
        w.append(alpha * T), m.append(t), d.append(np.float64(dl[k, 0]))
        T *= 1.0 - alpha
        Ts.append(T)
        if T < T_thresh:
            break
    return np.array(w), np.array(m), np.array(d), np.array(Ts)


def pairwise64(w, m, d):
    """The definition: numpy or torch float64."""
    lib = torch if torch.is_tensor(w) else np
    return (w[:, None] * w[None, :] * lib.abs(m[:, None] - m[None, :])).sum() + (d * w * w).sum() / 3


def prefix_form64(w, m, d):
    """The O(n) form (loss.py:29-76 per ray) and d dist / d w in closed form, numpy float64: -> (dist, v [K])."""
    wm = w * m
    Wpre, WMpre = np.cumsum(w) - w, np.cumsum(wm) - wm
    dist = (2 * w * (m * Wpre - WMpre)).sum() + (d * w * w).sum() / 3
    Wsuf, WMsuf = w.sum() - Wpre - w, wm.sum() - WMpre - wm
    v = 2 * (m * (Wpre - Wsuf) + (WMsuf - WMpre)) + (2 / 3) * d * w
    return dist, v


def grad_sigma_closed64(sig, dl, off, cnt, T_thresh=T_THRESH):
    """d dist / d sigma of one ray by the kernel's formula, numpy float64 [K]: d_k (v_k T_{k+1} - (2 dist - S_k))."""
    w, m, d, T = ray_weights64(sig, dl, off, cnt, T_thresh)
    dist, v = prefix_form64(w, m, d)
    return d * (v * T - (2 * dist - np.cumsum(v * w)))


def reference64(sig, dl, rays, T_thresh=T_THRESH, grad_dist=None):
    """The statement on a ragged batch: -> dict(dist [N], w_sum [N], wm_sum [N] (m counted from the ray's first sample), grad_sigmas [M],
    live [M] bool: the samples that count, stops {row: index of the last counting sample}), float64 numpy.  Outputs are indexed by ray id."""
    M, N = sig.shape[0], rays.shape[0]
    dist, w_sum, wm_sum = np.zeros(N), np.zeros(N), np.zeros(N)
    grad, live, stops = np.zeros(M), np.zeros(M, bool), {}
    g = np.ones(N) if grad_dist is None else np.asarray(grad_dist, np.float64)
    for n in range(N):
        idx, off, cnt = (int(v) for v in rays[n])
        if ray_is_empty(off, cnt, M):
            continue
        s = torch.tensor(sig[off:off + cnt].astype(np.float64), requires_grad=True)
        d0 = torch.tensor(dl[off:off + cnt, 0].astype(np.float64))
        d1 = torch.tensor(dl[off:off + cnt, 1].astype(np.float64))
        T, t, ws, ms = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), [], []
        for k in range(cnt):                      # the sample-order loop with its stop rule
            alpha = 1 - torch.exp(-s[k] * d0[k])
            t = t + d1[k]
            ws.append(alpha * T), ms.append(t)
            T = T * (1 - alpha)
            if float(T.detach()) < T_thresh:
                break
        K = len(ws)
        w, m = torch.stack(ws), torch.stack(ms)
        value = pairwise64(w, m, d0[:K])
        value.backward()
        dist[idx], w_sum[idx] = float(value.detach()), float(w.detach().sum())
        wm_sum[idx] = float((w * (m - m[0])).detach().sum())
        grad[off:off + cnt] = g[idx] * s.grad.numpy()
        live[off:off + K] = True
        stops[n] = K - 1
    return dict(dist=dist, w_sum=w_sum, wm_sum=wm_sum, grad_sigmas=grad, live=live, stops=stops)


# ------------------------------------------------------------------------------------------------ the per-op fp32 formulation
def per_op_fp32(sigmas, deltas, rays, T_thresh=T_THRESH):
    """Padded dense torch, fp32, on the tensors' device; sigmas may require grad.  -> dist [N] indexed by ray id (autograd reaches sigmas)."""
    M, N = sigmas.shape[0], rays.shape[0]
    idx, off, cnt = rays[:, 0].long(), rays[:, 1].long(), rays[:, 2].long()
    cnt = torch.where(off + cnt > M, torch.zeros_like(cnt), cnt)
    L = max(int(cnt.max()), 1) if N else 1
    k = torch.arange(L, device=sigmas.device)[None, :]
    valid = k < cnt[:, None]
    rows = (off[:, None] + k).clamp(max=max(M - 1, 0))
    sg = torch.where(valid, sigmas[rows], torch.zeros((), device=sigmas.device))
    d0 = torch.where(valid, deltas[rows, 0], torch.zeros((), device=sigmas.device))
    d1 = torch.where(valid, deltas[rows, 1], torch.zeros((), device=sigmas.device))
    alpha = 1 - torch.exp(-sg * d0)
    T_after = torch.cumprod(1 - alpha, dim=-1)
    T = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], dim=-1)
    w = torch.where(valid & ~(T < T_thresh), alpha * T, torch.zeros((), device=sigmas.device))
    m = torch.cumsum(d1, dim=-1)
    wm = w * m
    Wpre, WMpre = torch.cumsum(w, -1) - w, torch.cumsum(wm, -1) - wm          # loss.py:42-48
    per_row = (2 * w * (m * Wpre - WMpre) + (1 / 3) * d0 * w * w).sum(-1)
    return torch.zeros(N, dtype=sigmas.dtype, device=sigmas.device).index_add(0, idx, per_row)


# ------------------------------------------------------------------------------------------------ the test batch
@functools.lru_cache(maxsize=None)
def batch(kind="main"):
    """main: 48 rays, M ~ 3 000.  num_steps from STEPS; ray ids a permutation; the last row overruns M; one ray opaque by sample 5; one ray
    that crosses T_thresh at lane 15 of a 16-sample group and one at lane 0 of the next; deltas[:,1] of a ray's first sample is the ray's
    near distance, so absolute t reaches 80; a stretch of samples that no ray owns.
    long_first: the same samples with a 600-sample ray as row 0.  one: a single 33-sample ray.  -> dict of numpy arrays (never modified)."""
    if kind == "long_first":
        b = dict(batch("main"))
        first = int(np.argmax(b["rays"][:, 2] == 600))
        order = np.array([first] + [i for i in range(b["N"]) if i != first])
        b["rays"] = np.ascontiguousarray(b["rays"][order])
        b["forced"] = {int(np.nonzero(order == n)[0][0]): at for n, at in b["forced"].items()}
        b["over"] = int(np.nonzero(order == b["over"])[0][0])
        return b
    if kind == "one":
        m = batch("main")
        n = int(np.argmax(m["rays"][:, 2] == 33))
        off = int(m["rays"][n, 1])
        return dict(N=1, M=33, rays=np.array([[0, 0, 33]], np.int32), sig=m["sig"][off:off + 33].copy(), dl=m["dl"][off:off + 33].copy(),
                    gdist=m["gdist"][:1].copy(), forced={}, over=-1, gap=(0, 0))
    rng = np.random.default_rng(21)
    small = [s for s in STEPS if s < 100]
    counts = np.array(small * 4 + [100] * 9 + [600] * 2 + [17])              # 36 + 9 + 2 + 1 = 48 rows; the last one overruns M
    N = counts.shape[0]
    order = np.concatenate([rng.permutation(N - 1), [N - 1]])
    counts = counts[order]
    GAP = 150
    gap_row = 20                                                             # the unowned stretch lies in front of this row's samples
    offs = np.zeros(N, np.int64)
    at = 0
    for n in range(N - 1):
        if n == gap_row:
            gap = (at, at + GAP)
            at += GAP
        offs[n] = at
        at += counts[n]
    M = int(at) + 7                                                            # ... and seven more behind the last owned sample
    offs[N - 1] = M - 10                                                     # 17 samples from M - 10: skipped
    ids = rng.permutation(N)
    rays = np.stack([ids, offs, counts], 1).astype(np.int32)
    sig = (rng.random(M) * 40).astype(np.float32)
    d0 = rng.uniform(0.004, 0.02, M).astype(np.float32)
    d1 = (d0 * rng.uniform(0.9, 1.1, M)).astype(np.float32)
    hundred = [n for n in range(N - 1) if counts[n] == 100]
    translucent = rng.random(N) < 0.5
    translucent[hundred[:3]] = True                                          # the three forced rays below start translucent
    translucent[[n for n in range(N) if counts[n] == 600]] = [True, False]   # one long ray runs its length, one stops on the threshold
    for n in np.nonzero(translucent)[0]:
        sig[offs[n]:min(offs[n] + counts[n], M)] *= 0.03
    forced = {hundred[0]: 4, hundred[1]: 31, hundred[2]: 32}                 # row -> the sample that brings T below T_thresh
    for n, k in forced.items():
        sig[offs[n] + k] = 2000.0 / 0.8                                      # sigma d >= 10: T falls by e^-10 at least at this sample
        d0[offs[n] + k] = max(d0[offs[n] + k], 0.004)
    for n in range(N - 1):
        if counts[n]:
            d1[offs[n]] = 78.0 if counts[n] == 600 else rng.uniform(60.0, 79.0)    # the ray's near distance
    dl = np.stack([d0, d1], 1)
    gdist = (rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    return dict(N=N, M=M, rays=rays, sig=sig, dl=dl, gdist=gdist, forced=forced, over=N - 1, gap=gap)


@functools.lru_cache(maxsize=None)
def truth(kind="main"):
    """reference64 of batch(kind), computed once (never modified)."""
    b = batch(kind)
    return reference64(b["sig"], b["dl"], b["rays"], T_THRESH, b["gdist"])


def check_batch(b):
    """The conditions the GPU comparisons rely on, in float64; -> the smallest |T / T_thresh - 1| over every transmittance of the batch."""
    N, M, rays = b["N"], b["M"], b["rays"]
    worst = np.inf
    for n in range(N):
        _, off, cnt = (int(v) for v in rays[n])
        if ray_is_empty(off, cnt, M):
            continue
        T = np.cumprod(np.exp(-b["sig"][off:off + cnt].astype(np.float64) * b["dl"][off:off + cnt, 0].astype(np.float64)))
        worst = min(worst, float(np.abs(T / T_THRESH - 1).min()))
    assert worst > MARGIN, worst            # the cap on rays left out of a comparison is 0
    return worst
