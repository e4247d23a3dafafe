"""A float64 numpy statement of the palette extraction's front end, written from the reference's lines and scikit-learn's source -- what
palettenerf_amd.extract and csrc/extract.hip are tested against (tests/test_extract_host.py, tests/test_gpu_extract.py).

  accumulate   PaletteTrainer.extract_palette, palette/utils.py:1162-1186, and RGB_to_bin_index, palette/src/bindings.cpp:40-50
  kmeans       palette_extraction :209-226, run_kmeans :148-165, and scikit-learn 1.7's _kmeans_single_lloyd (sklearn/cluster/_kmeans.py:624-752,
               lloyd_iter_chunked_dense in _k_means_lloyd.pyx, _relocate_empty_clusters_dense / _average_centers / _center_shift in
               _k_means_common.pyx) WITH the relocation of emptied clusters

Everything after the stored pixel is float64.  scikit-learn's centring of the points (KMeans.fit subtracts X.mean) and its float32 rounding are
not part of the statement; neither changes the exact result."""
import numpy as np

FENCE = 2.0 ** -20          # a sample this close to a bin boundary may fall on either side in fp32 (the normalisation's error is a few 6e-8)
CLAMP_HI = float(np.float32(0.999))


def stored_pixels(view):
    """a stored view [..., C] (float32, float16 or uint8) as the loader's pixels: fp32 as stored, fp16 exactly, uint8 as float32(u) / 255 in float32"""
    view = np.asarray(view)
    if view.dtype == np.uint8:
        return (view.astype(np.float32) / np.float32(255)).astype(np.float64)
    return view.astype(np.float64)


def srgb_to_linear(x):
    return np.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def codes_of(c, bits):
    """RGB_to_bin_index: per channel floor(clamp(c, 0, 0.999f) * 2^bits), r most significant"""
    q = np.floor(np.clip(c, 0.0, CLAMP_HI) * float(1 << bits)).astype(np.int64)
    return (q[:, 0] << (2 * bits)) | (q[:, 1] << bits) | q[:, 2]


def near_fence(c, bits):
    """how many rows of c [n,3] have a channel within FENCE of a bin boundary k / 2^bits, k = 1 .. 2^bits - 1"""
    s = c * float(1 << bits)
    k = np.rint(s)
    on = (np.abs(s - k) < FENCE * float(1 << bits)) & (k >= 1) & (k <= (1 << bits) - 1)
    return int(on.any(axis=1).sum())


def accumulate(weights_sum, view, linear=False, thresh=0.5):
    """One view.  weights_sum [N] float32, view [H,W,C] or [N,C] as stored.  Returns {coarse [512], fine [32768] int64, total, B3, B5}: B = the
    valid samples within FENCE of a boundary of that grid."""
    ws = np.asarray(weights_sum, dtype=np.float32).reshape(-1)
    p = stored_pixels(view).reshape(ws.shape[0], -1)[:, :3]
    valid = ws > np.float32(thresh)                              # strict; a NaN compares false
    p = p[valid]
    if linear:
        p = srgb_to_linear(p)
    c = p + float(np.float32(0.05))
    c = c / np.sqrt((c * c).sum(axis=1, keepdims=True))
    out = {"total": int(valid.sum())}
    for bits, name in ((3, "coarse"), (5, "fine")):
        out[name] = np.bincount(codes_of(c, bits), minlength=1 << (3 * bits)).astype(np.int64)
        out["B%d" % bits] = near_fence(c, bits)
    return out


def bin_centers(bits):
    code = np.arange(1 << (3 * bits), dtype=np.int64)
    mask = (1 << bits) - 1
    return (np.stack([(code >> (2 * bits)) & mask, (code >> bits) & mask, code & mask], axis=1) + 0.5) / float(1 << bits)


def points_of(coarse, fine, total, tau=8e-3):
    """palette_extraction :209-222: (points [P,3], weights [P], init [K,3])"""
    coarse, fine = np.asarray(coarse, dtype=np.float64), np.asarray(fine, dtype=np.float64)
    heavy = coarse / float(total) > tau
    some = fine > 0
    return bin_centers(5)[some], fine[some] / float(total), bin_centers(3)[heavy]


def labels_of(X, centers):
    """argmin of ((x0-c0)^2 + (x1-c1)^2) + (x2-c2)^2, the first minimum"""
    d = (X[:, None, :] - centers[None, :, :]) ** 2
    return np.argmin((d[..., 0] + d[..., 1]) + d[..., 2], axis=1)


def lloyd(X, w, init, max_iter=300, tol=1e-4):
    """Returns {centers [K,3] (cluster order), labels [P], iterations, stop ('labels' | 'shift' | 'max_iter'), emptied: the iterations in which a
    cluster was relocated}."""
    X, w = np.asarray(X, dtype=np.float64), np.asarray(w, dtype=np.float64)
    centers = np.array(init, dtype=np.float64)
    K = len(centers)
    tol_abs = np.mean(np.var(X, axis=0)) * tol                  # _tolerance
    labels_old = np.full(len(X), -1)
    stop, emptied = "max_iter", []
    for i in range(max_iter):
        labels = labels_of(X, centers)
        sums, wk = np.zeros((K, 3)), np.zeros(K)
        for k in range(K):
            sel = labels == k
            sums[k] = (w[sel, None] * X[sel]).sum(axis=0)
            wk[k] = w[sel].sum()
        empty = np.where(wk == 0)[0]
        if len(empty):
            emptied.append(i)
            dist = ((X - centers[labels]) ** 2).sum(axis=1)
            far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
            if dist.max() != 0:
                for idx in range(len(empty)):
                    f, new = far[idx], empty[idx]
                    old = labels[f]
                    sums[old] -= X[f] * w[f]
                    sums[new] = X[f] * w[f]
                    wk[new] = w[f]
                    wk[old] -= w[f]
        heaviest = np.argmax(wk)
        for k in range(K):                                       # _average_centers, in place and in order
            if wk[k] > 0:
                sums[k] *= 1.0 / wk[k]
            else:
                sums[k] = sums[heaviest]
        shift = np.sqrt(((sums - centers) ** 2).sum(axis=1))
        centers = sums
        if np.array_equal(labels, labels_old):
            stop = "labels"
            break
        if (shift ** 2).sum() <= tol_abs:
            stop = "shift"
            break
        labels_old = labels
    if stop != "labels":
        labels = labels_of(X, centers)
    return {"centers": centers, "labels": labels, "iterations": i + 1, "stop": stop, "emptied": emptied}


def run_kmeans(X, w, init, max_iter=300, tol=1e-4):
    """run_kmeans :148-165 over lloyd: the statement's result with centres and weights by descending weight, ties to the lower cluster index"""
    r = lloyd(X, w, init, max_iter, tol)
    cw = np.array([w[r["labels"] == k].sum() for k in range(len(init))])
    order = np.argsort(-cw, kind="stable")
    return dict(r, sorted_centers=r["centers"][order], center_weights=cw[order], order=order)


def parent_of(code):
    """the coarse bin a fine bin lies in"""
    code = np.asarray(code)
    return (((code >> 12) & 7) << 6) | (((code >> 7) & 7) << 3) | ((code >> 2) & 7)


def seeded_tables(seed, P, K, lo=1, hi=10 ** 7):
    """Consistent count tables with exactly P non-empty fine bins, drawn anywhere in the colour cube with log-uniform counts in [lo, hi]; the
    coarse table is the sum over each coarse bin's 64 fine bins, and tau lies halfway between the K-th and the (K+1)-th heaviest coarse weight,
    so that exactly K coarse bins become centres.  Returns (coarse, fine, total, tau).  Points outside the K heavy bins move between clusters
    for several iterations, as an extraction's do."""
    rng = np.random.default_rng(seed)
    while True:
        chosen = rng.choice(32768, size=P, replace=False)
        fine = np.zeros(32768, dtype=np.int64)
        fine[chosen] = np.floor(np.exp(rng.uniform(np.log(lo), np.log(hi + 1), size=P))).astype(np.int64).clip(lo, hi)
        coarse = np.bincount(parent_of(np.arange(32768)), weights=fine, minlength=512).astype(np.int64)
        total = int(fine.sum())
        heavy = np.sort(coarse[coarse > 0] / total)[::-1]
        if len(heavy) < K or (len(heavy) > K and heavy[K - 1] == heavy[K]):
            continue
        tau = (heavy[K - 1] + (heavy[K] if len(heavy) > K else 0.0)) / 2
        return coarse, fine, total, float(tau)


def emptied_tables():
    """Six points on the r axis (g = b = 0), in units of 1/32: 0.5 (1), 3.5 (1000) | 4.5 (10), 7.5 (10) | 8.5 (1000), 11.5 (1): three coarse bins,
    three centres at 2, 6, 10.  Iteration 0 labels them by coarse bin and moves the outer centres to 3.497 and 8.503, the middle one stays at 6;
    in iteration 1 the middle cluster's points are nearer to the outer centres (1.0 against 1.5) and it is left empty."""
    fine = np.zeros(32768, dtype=np.int64)
    for q, c in ((0, 1), (3, 1000), (4, 10), (7, 10), (8, 1000), (11, 1)):
        fine[q << 10] = c
    coarse = np.bincount(parent_of(np.arange(32768)), weights=fine, minlength=512).astype(np.int64)
    return coarse, fine, int(fine.sum()), 8e-3
