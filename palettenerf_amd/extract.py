"""Step 2 of the reference's workflow on the device, between the NeRF stage and the PaletteNeRF stage: `PaletteTrainer.extract_palette`
(palette/utils.py:1135-1200) and `palette_extraction` (:167-254).

The reference renders every training view, keeps four per-pixel arrays for the pixels with weights_sum > 0.5, concatenates them over all views,
copies them to the host, histograms them twice on one core and runs scikit-learn's weighted KMeans on the non-empty fine bins.  All the later
stages need from that are two histograms (512 + 32 768 counts) and K <= 124 colour centres with their weights.  Here a view is ONE launch that
folds it into both histograms (`pnr_extract_accumulate`: integer counts, so exact and independent of order), the whole weighted k-means is ONE
launch (`pnr_extract_kmeans`: float64, fixed summation order), the hull simplification that turns the centres into the 4..10 palette colours is
ONE launch of one workgroup (`pnr_hull_simplify`, include/pnr_hull.h: every hull by brute force, every edge's linear program by vertex
enumeration, float64, fixed order), and the weight LUT is ONE launch (`pnr_lut_weights`).  A few kilobytes are read back.

    palette, lut, res = extract.extract_palette(model, poses, intrinsics, H, W, trainset, palette_model=palette_model, normalize_input=True)

or step by step:

    res = extract.extract_centers(model, poses, intrinsics, H, W, trainset)            # or an image stack, host or device
    palette = extract.simplify_hull(res["centers"], res["center_weights"])             # Hull_Simplification_posternerf
    extract.initialize_from_extraction(palette_model, palette, normalize_input=True)   # the weight LUT: stays on the device

`simplify_hull_per_op` is the hull simplification on the host in the reference's line order with scipy (ConvexHull, linprog(method="highs")),
kept to measure and test against and to finish what the kernel hands over by status (a coplanar facet, a flat set, an edge with more related
faces than the compiled cap).  `save_palette` / `load_palette` write and read the reference's palette files.  The weight LUT -- the
Tan-2016/2018 "ASAP" weights of the 32 768 five-bit bins, palette/utils.py:235-245 -- is
`weight_lut` (`pnr_lut_weights`: hull, projection and barycentrics in float64, one launch, nothing uploaded but the palette), and
`palette_weights` is the same for any device array of colours.  `weight_lut_per_op` is the same statement in numpy on the host, kept to
measure and test against.  The `extract-radiance-raw.png` debugging image of palette/utils.py:196-203 needs every sample on the host and is
not produced, nor are the hull simplification's OBJ files and `extract-palette.png`.  `extract_centers_per_op` is the reference's own sequence,
kept to measure and test against.  There is no fallback: on a CPU tensor or without the HIP library the device functions raise."""
import ctypes
import itertools

import numpy as np
import torch

from . import _lib
from ._torch_glue import stream_ptr

_FORMAT_OF = {torch.float32: _lib.IMAGE_FP32, torch.float16: _lib.IMAGE_FP16, torch.uint8: _lib.IMAGE_UINT8}
_BINS = {3: _lib.EXTRACT_COARSE_BINS, 5: _lib.EXTRACT_FINE_BINS}
_STATUS_TEXT = {_lib.EXTRACT_NO_CENTER: "no coarse bin is heavier than tau (K = 0): nothing to cluster",
                _lib.EXTRACT_TOO_MANY: f"more than {_lib.EXTRACT_MAX_K} coarse bins are heavier than tau (K above the compiled cap)",
                _lib.EXTRACT_FEW_POINTS: "fewer non-empty fine bins than centres (P < K)"}


def bin_centers_of(bits):
    """The reference's bin centres (palette/src/bindings.cpp:77-87) as float32 [2^(3 bits), 3]: (code + 0.5) / 2^bits per channel, r most significant."""
    code = np.arange(1 << (3 * bits), dtype=np.int64)
    mask = (1 << bits) - 1
    c = np.stack([(code >> (2 * bits)) & mask, (code >> bits) & mask, code & mask], axis=1).astype(np.float32)
    return (c + np.float32(0.5)) / np.float32(1 << bits)


class RadianceHistogram:
    """The two count tables of the extraction (3 and 5 bits per channel) and the number of valid samples, on the device as int64.
    `update` is one launch and reads nothing back; `counts`, `bin_weights`, `bin_centers` are device tensors; `total` is a read-back."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RadianceHistogram needs the HIP path (a CUDA/HIP device); there is no CPU fallback")
        self._buf = torch.zeros(_BINS[3] + _BINS[5] + 1, dtype=torch.int64, device=self.device)      # coarse | fine | total

    def clear(self):
        self._buf.zero_()

    def counts(self, bits):
        """The int64 table of `bits` (3 or 5) bits per channel, a view of the live buffer."""
        if bits not in _BINS:
            raise ValueError("RadianceHistogram: the tables have 3 and 5 bits per channel")
        return self._buf[:_BINS[3]] if bits == 3 else self._buf[_BINS[3]:_BINS[3] + _BINS[5]]

    @property
    def total_tensor(self):
        return self._buf[_BINS[3] + _BINS[5]:]

    @property
    def total(self):
        """The number of valid samples so far (synchronises: one int64 read back)."""
        return int(self.total_tensor.item())

    def bin_weights(self, bits):
        """compute_RGB_histogram's first result for unit weights: float64 [2^(3 bits)] on the device (the counts, not normalised)."""
        return self.counts(bits).to(torch.float64)

    def bin_centers(self, bits):
        """compute_RGB_histogram's second result: float32 [2^(3 bits), 3] on the device."""
        if bits not in _BINS:
            raise ValueError("RadianceHistogram: the tables have 3 and 5 bits per channel")
        return torch.from_numpy(bin_centers_of(bits)).to(self.device)

    def load_counts(self, coarse, fine, total=None):
        """Replace the tables (a saved run, a test): coarse [512], fine [32768] integer counts; total defaults to coarse.sum()."""
        coarse = torch.as_tensor(np.asarray(coarse), dtype=torch.int64).reshape(-1)
        fine = torch.as_tensor(np.asarray(fine), dtype=torch.int64).reshape(-1)
        if coarse.numel() != _BINS[3] or fine.numel() != _BINS[5] or bool((coarse < 0).any()) or bool((fine < 0).any()):
            raise ValueError("RadianceHistogram.load_counts: coarse [512] and fine [32768] non-negative counts")
        total = int(coarse.sum()) if total is None else int(total)
        self._buf.copy_(torch.cat([coarse, fine, torch.tensor([total], dtype=torch.int64)]).to(self.device))
        return self

    def update(self, weights_sum, pixels, linear=False, thresh=0.5):
        """Fold one view in: weights_sum [H W] fp32 on the device (the frame's output, read where it lies), pixels [H,W,3 or 4] (or [N,3 or 4]) as
        fp32, fp16 or uint8 -- the ground truth as TrainSet stores it; rows may be padded, alpha is not read; a host array is uploaded.
        valid = weights_sum > thresh; linear: srgb_to_linear on the pixel first.  ONE launch, no synchronisation."""
        if not torch.is_tensor(pixels):
            pixels = torch.from_numpy(np.asarray(pixels))
        if pixels.dtype == torch.float64:
            pixels = pixels.to(torch.float32)
        if pixels.dtype not in _FORMAT_OF:
            raise ValueError(f"RadianceHistogram.update: pixels must be float32, float16 or uint8, got {pixels.dtype}")
        if pixels.ndim == 2:
            pixels = pixels[None]
        if pixels.ndim != 3 or pixels.shape[2] not in (3, 4):
            raise ValueError(f"RadianceHistogram.update: pixels must be [H,W,3 or 4] or [N,3 or 4], got {tuple(pixels.shape)}")
        if pixels.device != self.device:
            pixels = pixels.to(self.device, non_blocking=True)
        H, W, C = pixels.shape
        if pixels.numel() and (pixels.stride(2) != 1 or pixels.stride(1) != C or (H > 1 and pixels.stride(0) < W * C)):
            pixels = pixels.contiguous()
        if not torch.is_tensor(weights_sum) or weights_sum.dtype != torch.float32 or weights_sum.device != self.device:
            raise RuntimeError("RadianceHistogram.update: weights_sum must be a float32 tensor on the histogram's device")
        if weights_sum.numel() != H * W:
            raise ValueError(f"RadianceHistogram.update: weights_sum has {weights_sum.numel()} values, the view {H} x {W} pixels")
        weights_sum = weights_sum.detach()
        if not weights_sum.is_contiguous():
            weights_sum = weights_sum.contiguous()
        a = _lib.ExtractAccumulateArgs()
        a.H, a.W, a.channels, a.image_format = H, W, C, _FORMAT_OF[pixels.dtype]
        a.weights_sum, a.pixels = weights_sum.data_ptr(), pixels.data_ptr()
        a.row_stride_bytes = (pixels.stride(0) if H > 1 else W * C) * pixels.element_size()
        a.linear, a.thresh = int(bool(linear)), float(thresh)
        a.counts_coarse, a.counts_fine, a.total = self.counts(3).data_ptr(), self.counts(5).data_ptr(), self.total_tensor.data_ptr()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pnr_extract_accumulate(ctypes.byref(a), stream_ptr()), "pnr_extract_accumulate")
        return self


def _view_source(images, device):
    """view i of the ground truth -> a [H,W,C] tensor: a TrainSet's device-resident stack and a device stack are indexed (a view, no copy);
    a host stack is uploaded view by view."""
    stack = getattr(images, "images", None) if not torch.is_tensor(images) and not isinstance(images, np.ndarray) else None
    if stack is not None:                                   # a TrainSet
        return lambda i: stack[i]
    if torch.is_tensor(images) and images.is_cuda:
        return lambda i: images[i]
    return lambda i: torch.as_tensor(np.asarray(images[i]) if not torch.is_tensor(images) else images[i]).to(device, non_blocking=True)


def _render_kwargs(model, render_kwargs):
    kw = dict(render_kwargs, bg_color=None, perturb=False)              # test_step's defaults (palette/utils.py:938-946)
    if hasattr(model, "num_basis"):
        kw.setdefault("gui_mode", True)                                # only weights_sum is read: the frame without the per-basis maps (pass gui_mode=False for test_step's own)
    return kw


def radiance_histograms(model, poses, intrinsics, H, W, images, linear=False, thresh=0.5, hist=None, frames_in_flight=1, **render_kwargs):
    """The loop of extract_palette (palette/utils.py:1157-1194) for a NeRF or a PaletteNeRF model: for every view, rays on the device, a frame
    with bg_color = None and perturb = False through pipeline.render_queue (frame i + 1 is prepared under frame i; frames_in_flight > 1:
    pipeline.FramesInFlight instead), then ONE launch that folds the view into both histograms.  images: [n,H,W,3 or 4] host or device stack
    (fp32, fp16 or uint8), or a TrainSet, whose device-resident stack is read in place.  linear: the scene's colour space is linear
    (TrainSet.color_space == "linear").  Nothing is read back.  Returns the RadianceHistogram (`hist`, or a new one)."""
    from . import pipeline
    from . import rays as prays
    device = next(model.parameters()).device
    poses = torch.as_tensor(poses, dtype=torch.float32).reshape(-1, 4, 4).to(device)
    n = poses.shape[0]
    if hist is None:
        hist = RadianceHistogram(device)
    view = _view_source(images, device)
    kw = _render_kwargs(model, render_kwargs)

    def rays_of(i):
        return prays.rays_from_indices(poses[i:i + 1], intrinsics, H, W, None)

    def use(i, r):
        hist.update(r["weights_sum"].reshape(-1), view(i), linear=linear, thresh=thresh)

    if int(frames_in_flight) > 1 and n > 1:
        fif = pipeline.FramesInFlight(model, min(int(frames_in_flight), n), device)
        try:
            fif.render(rays_of, n, consume=use, **kw)
        finally:
            fif.close()
    else:
        pipeline.render_queue(model, rays_of, n, consume=use, **kw)
    return hist


# ---------------------------------------------------------------- k-means on the host: the per-op leg and the emptied-cluster hand-over
def _labels_of(X, centers):
    d = X[:, None, :] - centers[None, :, :]
    d *= d
    return np.argmin((d[..., 0] + d[..., 1]) + d[..., 2], axis=1)


def lloyd_host(X, w, init, max_iter=300, tol=1e-4):
    """scikit-learn's _kmeans_single_lloyd (1.7: sklearn/cluster/_kmeans.py, _k_means_lloyd.pyx, _k_means_common.pyx) in numpy float64, WITH the
    relocation of emptied clusters (_relocate_empty_clusters_dense) -- what pnr_extract_kmeans hands over when a cluster loses its points, and what
    the per-op leg runs where scikit-learn is not installed.  X [P,3], w [P], init [K,3].  Returns (centers [K,3], labels [P], iterations, stop),
    stop in ("labels", "shift", "max_iter").  scikit-learn's centring of X and its float32 rounding are not imitated."""
    X, w = np.asarray(X, dtype=np.float64), np.asarray(w, dtype=np.float64)
    centers = np.array(init, dtype=np.float64)
    K = centers.shape[0]
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    labels_old = np.full(X.shape[0], -1, dtype=np.int64)
    stop, it = "max_iter", 0
    for it in range(int(max_iter)):
        labels = _labels_of(X, centers)
        sums, wk = np.zeros((K, 3)), np.zeros(K)
        np.add.at(sums, labels, w[:, None] * X)
        np.add.at(wk, labels, w)
        empty = np.where(wk == 0)[0]
        if empty.size:                                           # _relocate_empty_clusters_dense
            dist = ((X - centers[labels]) ** 2).sum(axis=1)
            far = np.argpartition(dist, -empty.size)[:-empty.size - 1:-1]
            if dist.max() != 0:
                for new, f in zip(empty, far):
                    old = labels[f]
                    sums[old] -= X[f] * w[f]
                    sums[new] = X[f] * w[f]
                    wk[new] = w[f]
                    wk[old] -= w[f]
        new = sums
        heaviest = int(np.argmax(wk))
        for k in range(K):                                       # _average_centers, in its order
            new[k] = new[k] * (1.0 / wk[k]) if wk[k] > 0 else new[heaviest]
        shift = np.sqrt(((new - centers) ** 2).sum(axis=1))      # _center_shift, squared again by the caller
        centers = new
        if np.array_equal(labels, labels_old):
            stop = "labels"
            break
        if (shift ** 2).sum() <= tol_abs:
            stop = "shift"
            break
        labels_old = labels
    if stop != "labels":
        labels = _labels_of(X, centers)
    return centers, labels, it + 1, stop


def sort_centers(centers, labels, w):
    """run_kmeans' tail (palette/utils.py:159-165): the weight of every cluster, both sorted by descending weight, ties to the lower cluster index."""
    K = centers.shape[0]
    cw = np.array([np.sum(w[labels == k]) for k in range(K)], dtype=np.float64)
    order = np.argsort(-cw, kind="stable")
    return centers[order], cw[order]


def points_of(counts_coarse, counts_fine, total, tau):
    """palette/utils.py:209-222 from the count tables: (points [P,3], weights [P], init [K,3]) in float64."""
    coarse, fine = np.asarray(counts_coarse, dtype=np.float64), np.asarray(counts_fine, dtype=np.float64)
    total = float(total)
    heavy = coarse / total > tau if total > 0 else np.zeros(coarse.shape, dtype=bool)
    some = fine > 0
    return bin_centers_of(5)[some].astype(np.float64), fine[some] / total, bin_centers_of(3)[heavy].astype(np.float64)


def kmeans_centers(hist, tau=8e-3, max_iter=300, tol=1e-4, return_labels=False):
    """The rest of palette_extraction up to run_kmeans' return, from a RadianceHistogram: ONE launch and ONE read-back of 4 KB.
    Returns (centers [K,3] float64, center_weights [K] float64, info): the arguments of Hull_Simplification_posternerf(centers, ...,
    pixel_counts=center_weights).  info: K, P, iterations, stop ("labels", "shift" or "max_iter"), emptied (False, or the iteration at which a
    cluster lost its points: from there the loop was finished on the host with scikit-learn's relocation rule, lloyd_host), and with
    return_labels the final label of every point (before the sort), a second read-back.  K = 0, K > 128 and P < K raise RuntimeError."""
    lib = _lib.load()
    dev = hist.device
    kmax = _lib.EXTRACT_MAX_K
    out = torch.empty(4 * kmax + 4, dtype=torch.float64, device=dev)                 # centres | weights | info (8 int32)
    labels = torch.empty(_BINS[5], dtype=torch.int32, device=dev) if return_labels else None
    ws_bytes = int(lib.pnr_extract_kmeans_workspace_bytes())
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    a = _lib.ExtractKmeansArgs()
    a.counts_coarse, a.counts_fine, a.total = hist.counts(3).data_ptr(), hist.counts(5).data_ptr(), hist.total_tensor.data_ptr()
    a.tau, a.tol, a.max_iter = float(tau), float(tol), int(max_iter)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.centers, a.center_weights, a.info = out.data_ptr(), out.data_ptr() + 8 * 3 * kmax, out.data_ptr() + 8 * 4 * kmax
    a.labels = None if labels is None else labels.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.pnr_extract_kmeans(ctypes.byref(a), stream_ptr()), "pnr_extract_kmeans")
    host = out.cpu().numpy()
    K, P, iters, stop, status = (int(v) for v in host[4 * kmax:].view(np.int32)[:5])
    if status in _STATUS_TEXT:
        raise RuntimeError(f"pnr_extract_kmeans: {_STATUS_TEXT[status]} (K = {K}, P = {P}, tau = {tau})")
    info = {"K": K, "P": P, "iterations": iters, "stop": _lib.EXTRACT_STOP[stop], "emptied": False}
    centers, cw = host[:3 * K].reshape(K, 3).copy(), host[3 * kmax:3 * kmax + K].copy()
    lab = None if labels is None else labels[:P].cpu().numpy().astype(np.int64)
    if status == _lib.EXTRACT_EMPTIED:
        buf = hist._buf.cpu().numpy()
        X, w, _ = points_of(buf[:_BINS[3]], buf[_BINS[3]:_BINS[3] + _BINS[5]], buf[-1], tau)
        c, lab, n, stop = lloyd_host(X, w, centers, max_iter=int(max_iter) - iters, tol=tol)
        centers, cw = sort_centers(c, lab, w)
        info.update(iterations=iters + n, stop=stop, emptied=iters)
    if return_labels:
        info["labels"] = lab
    return centers, cw, info


def _result(centers, cw, info, coarse, fine, total):
    total = float(total)
    return {"centers": centers, "center_weights": cw, "hist_coarse": np.asarray(coarse, dtype=np.float64) / total,
            "hist_fine": np.asarray(fine, dtype=np.float64) / total, "hist_rgb": bin_centers_of(5), "total": int(total), "info": info}


def extract_centers(model, poses, intrinsics, H, W, images, linear=False, thresh=0.5, tau=8e-3, max_iter=300, tol=1e-4, frames_in_flight=1,
                    **render_kwargs):
    """radiance_histograms + kmeans_centers.  Returns a dict: centers [K,3] and center_weights [K] (float64, by descending weight), hist_coarse
    [512] and hist_fine [32768] (float64, the two histograms over the number of valid samples), hist_rgb [32768,3] (float32: the 5-bit bin
    centres the reference's weight-LUT step reads, palette/utils.py:235), total, info (kmeans_centers)."""
    hist = radiance_histograms(model, poses, intrinsics, H, W, images, linear=linear, thresh=thresh, frames_in_flight=frames_in_flight, **render_kwargs)
    centers, cw, info = kmeans_centers(hist, tau=tau, max_iter=max_iter, tol=tol)
    buf = hist._buf.cpu().numpy()
    return _result(centers, cw, info, buf[:_BINS[3]], buf[_BINS[3]:_BINS[3] + _BINS[5]], buf[-1])


_SAVED = ("centers", "center_weights", "hist_coarse", "hist_fine", "hist_rgb")


def save_centers(path, result):
    """The arrays of an extract_centers result (and its total) as one .npz."""
    np.savez(path, total=np.int64(result["total"]), **{k: np.asarray(result[k]) for k in _SAVED})


def load_centers(path):
    with np.load(path) as z:
        out = {k: z[k] for k in _SAVED}
        out["total"] = int(z["total"])
    return out


def _pixels_float(t):
    """a stored view as the loader's fp32 pixels: uint8 / 255, fp16 converted exactly"""
    return t.to(torch.float32) / 255 if t.dtype == torch.uint8 else t.to(torch.float32)


def extract_centers_per_op(model, poses, intrinsics, H, W, images, linear=False, thresh=0.5, tau=8e-3, max_iter=300, tol=1e-4, kmeans="auto",
                           **render_kwargs):
    """The reference's own sequence (palette/utils.py:1157-1200, :189-226), op by op -- what extract_centers is measured and tested against: per
    view the torch expressions and a boolean-mask gather, torch.cat over the views and .cpu(), compute_RGB_histogram twice on the samples, and
    sklearn.cluster.KMeans where it can be imported (otherwise, or with kmeans="host", lloyd_host in float64).  Returns extract_centers' dict."""
    from . import palette_utils
    from . import rays as prays
    device = next(model.parameters()).device
    poses = torch.as_tensor(poses, dtype=torch.float32).reshape(-1, 4, 4).to(device)
    view = _view_source(images, device)
    kw = _render_kwargs(model, render_kwargs)
    kept = []
    with torch.no_grad():
        for i in range(poses.shape[0]):
            ro, rd = prays.rays_from_indices(poses[i:i + 1], intrinsics, H, W, None)
            r = model.render(ro, rd, **kw)
            preds = _pixels_float(view(i))[..., :3].reshape(-1, 3)
            if linear:
                preds = torch.where(preds < 0.04045, preds / 12.92, ((preds + 0.055) / 1.055) ** 2.4)
            norm = preds + 0.05
            norm = norm / norm.norm(dim=-1, p=2, keepdim=True)
            kept.append(norm[r["weights_sum"].reshape(-1) > thresh])
        colors = torch.cat(kept, dim=0).detach().cpu().numpy()
    weights = np.ones_like(colors[..., 0])
    coarse, centers_coarse = palette_utils.compute_RGB_histogram(colors, weights, 3)
    total = np.sum(coarse)
    fine, centers_fine = palette_utils.compute_RGB_histogram(colors, weights, 5)
    heavy, some = coarse / total > tau, fine > 0
    X, w, init = centers_fine[some], fine[some] / total, centers_coarse[heavy]
    if init.shape[0] == 0 or X.shape[0] < init.shape[0]:
        raise RuntimeError(f"extract_centers_per_op: K = {init.shape[0]} centres for P = {X.shape[0]} points")
    KMeans = None
    if kmeans != "host":
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            pass
    if KMeans is not None:
        km = KMeans(n_clusters=init.shape[0], init=init, max_iter=max_iter, tol=tol).fit(X=X, sample_weight=w)
        c, labels, n, stop = km.cluster_centers_.astype(np.float64), km.labels_, km.n_iter_, None
    else:
        c, labels, n, stop = lloyd_host(X, w, init, max_iter=max_iter, tol=tol)
    centers, cw = sort_centers(c, labels, w)
    info = {"K": init.shape[0], "P": X.shape[0], "iterations": int(n), "stop": stop, "emptied": False}
    return _result(centers, cw, info, coarse, fine, total)


# ---------------------------------------------------------------- the weight LUT: hull projection and barycentrics (pnr_lut_weights)
_LUT_STATUS_TEXT = {_lib.LUT_FLAT: "the palette has fewer than four non-coplanar colours: there is no hull",
                    _lib.LUT_COPLANAR: "a face plane of the palette's hull carries a fourth colour within 1e-9: the triangulation of that "
                                       "facet, and with it the weights, would be a choice"}
_PLANE_EPS, _OUTSIDE_EPS = 1e-9, 1e-8


def _palette_rows(palette):
    p = np.asarray(palette.detach().cpu() if torch.is_tensor(palette) else palette, dtype=np.float64).reshape(-1, 3)
    if not _lib.LUT_MIN_M <= p.shape[0] <= _lib.LUT_MAX_M:
        raise ValueError(f"a palette of {_lib.LUT_MIN_M}..{_lib.LUT_MAX_M} colours is needed, got {p.shape[0]}")
    return np.ascontiguousarray(p)


def _launch_lut(palette, device, points, normalize_input, want64, want32):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the palette weights need the HIP path (a CUDA/HIP device); there is no CPU fallback")
    rows = _palette_rows(palette)
    M = rows.shape[0]
    pal = torch.from_numpy(rows).to(device)
    a = _lib.LutWeightsArgs()
    a.palette, a.M, a.normalize_input = pal.data_ptr(), M, int(bool(normalize_input))
    if points is None:
        N = _lib.EXTRACT_FINE_BINS
        a.points, a.points_format, a.point_stride = None, _lib.LUT_POINTS_BINS, 3
        shape32 = (1, M, 32, 32, 32)
    else:
        N = points.shape[0]
        a.points, a.point_stride = points.data_ptr(), points.stride(0) if N > 1 else 3
        a.points_format = _lib.LUT_POINTS_FP32 if points.dtype == torch.float32 else _lib.LUT_POINTS_FP64
        shape32 = (N, M)
    a.N = N
    info = torch.zeros(4, dtype=torch.int32, device=device)
    w64 = torch.empty(N, M, dtype=torch.float64, device=device) if want64 else None
    w32 = torch.empty(shape32, dtype=torch.float32, device=device) if want32 else None
    a.weights64 = None if w64 is None else w64.data_ptr()
    a.lut32 = None if w32 is None else w32.data_ptr()
    a.info = info.data_ptr()
    with torch.cuda.device(device):
        _lib.check(_lib.load().pnr_lut_weights(ctypes.byref(a), stream_ptr()), "pnr_lut_weights")
    status = int(info[0].item())
    if status in _LUT_STATUS_TEXT:
        raise RuntimeError(f"pnr_lut_weights: {_LUT_STATUS_TEXT[status]}")
    return w64, w32


def palette_weights(points, palette, out_dtype=torch.float64, normalize_input=False):
    """The Tan-2016/2018 "ASAP" weights of `points` [...,3] (a float32 or float64 tensor on the device; a 2-D view with a row stride is read
    in place) against `palette` [M,3], 4 <= M <= 16: [...,M] in out_dtype, float64 or float32 (the float64 result rounded once).  ONE launch.
    normalize_input: every point becomes (c + 0.05) / |c + 0.05| first.  A flat palette or a hull with a coplanar fourth colour raises."""
    if not torch.is_tensor(points) or not points.is_cuda or points.dtype not in (torch.float32, torch.float64) or points.shape[-1] != 3:
        raise RuntimeError("palette_weights: points must be a float32 or float64 [...,3] tensor on the device; there is no CPU fallback")
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError("palette_weights: out_dtype is torch.float64 or torch.float32")
    lead = points.shape[:-1]
    p = points.detach()
    if p.ndim != 2:
        p = p.reshape(-1, 3)
    if p.shape[0] > 1 and (p.stride(1) != 1 or p.stride(0) < 3):
        p = p.contiguous()
    elif p.shape[0] == 1 and p.stride(1) != 1:
        p = p.contiguous()
    if p.shape[0] >= 1 << 32:
        raise ValueError("palette_weights: more than 2^32 - 1 points")
    if p.shape[0] == 0:
        return torch.empty(*lead, _palette_rows(palette).shape[0], dtype=out_dtype, device=p.device)
    w64, w32 = _launch_lut(palette, p.device, p, normalize_input, out_dtype == torch.float64, out_dtype == torch.float32)
    out = w64 if out_dtype == torch.float64 else w32
    return out.reshape(*lead, out.shape[-1])


def weight_lut(palette, normalize_input=False, device="cuda", return_weights64=False):
    """The `hist_weights` table of palette/utils.py:235-245 as the model keeps it: float32 [1,M,32,32,32] on the device, the palette weights of the
    32 768 five-bit bin centres (with normalize_input, of (c + 0.05) / |c + 0.05|: --use_normalized_palette).  ONE launch that generates the bin
    centres itself; only the palette is uploaded and only the status word is read back.  return_weights64: also the float64 [32768,M] results
    the table was rounded from."""
    w64, w32 = _launch_lut(palette, device, None, normalize_input, bool(return_weights64), True)
    return (w32, w64) if return_weights64 else w32


def initialize_from_extraction(model, palette, normalize_input=False):
    """main_palette.py:138-141 + :217 without the reference's hist_weights.npz: the LUT of `palette` on the model's device, handed to
    model.initialize_palette in the layout the model keeps (no host round trip, no [32,32,32,M] numpy).  Returns the LUT."""
    rows = _palette_rows(palette)
    device = next(model.parameters()).device
    lut = weight_lut(rows, normalize_input=normalize_input, device=device)
    model.initialize_palette(rows, hist_lut=lut)
    return lut


def load_palette(path):
    """The palette a hull simplification wrote (the reference's, or save_palette): `palette.npz` / `*-palette.npz` (key 'palette') or `*-palette.txt` (one colour a
    line, three numbers: write_palette_txt, rgbsg/hull_simplification_posternerf.py:86-95).  Returns float64 [M,3]."""
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            p = np.asarray(z["palette"], dtype=np.float64)
    else:
        with open(path) as f:
            p = np.array([[float(v) for v in line.split()] for line in f if line.strip()], dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] == 0:
        raise ValueError(f"load_palette: {path} does not hold an [M,3] palette")
    return p


def lut_to_hist_weights(lut):
    """[1,M,R,G,B] (the model's layout, tensor or array) -> the reference's host table [R,G,B,M] float64."""
    a = lut.detach().cpu().numpy() if torch.is_tensor(lut) else np.asarray(lut)
    if a.ndim != 5 or a.shape[0] != 1:
        raise ValueError("lut_to_hist_weights: a [1,M,R,G,B] table is needed")
    return np.ascontiguousarray(np.transpose(a[0], (1, 2, 3, 0))).astype(np.float64)


def save_lut(path, lut):
    """A LUT as the reference's `hist_weights.npz` (key 'hist_weights', [32,32,32,M] float64): main_palette.py:140 reads it as it reads its
    own.  lut: weight_lut's [1,M,32,32,32] tensor, or a [32,32,32,M] host table."""
    a = lut.detach().cpu().numpy() if torch.is_tensor(lut) else np.asarray(lut)
    np.savez(path, hist_weights=lut_to_hist_weights(a) if a.ndim == 5 else a.astype(np.float64))


def load_lut(path, device=None):
    """`hist_weights.npz`, the reference's or save_lut's: the [32,32,32,M] float64 host table (initialize_palette's `hist_weights`), or with
    `device` the float32 [1,M,32,32,32] tensor there (initialize_palette's `hist_lut`)."""
    with np.load(path) as z:
        hw = np.asarray(z["hist_weights"], dtype=np.float64)
    if hw.ndim != 4:
        raise ValueError(f"load_lut: {path} does not hold an [R,G,B,M] table")
    if device is None:
        return hw
    return torch.as_tensor(hw).float().permute(3, 0, 1, 2).unsqueeze(0).contiguous().to(device)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def palette_hull(palette):
    """The hull of pnr_lut_weights in numpy float64: (order [M], V [M,3] = palette[order], faces [F,3] ascending triples of V, normals [F,3]
    unit and outward).  RuntimeError for a flat palette and for a coplanar fourth colour, with the device call's texts."""
    P = _palette_rows(palette)
    M = P.shape[0]
    order = np.argsort((np.abs(P[:, 0]) + np.abs(P[:, 1])) + np.abs(P[:, 2]), kind="stable")
    V = P[order]
    faces, normals, nonflat, coplanar = [], [], False, False
    for i, j, k in itertools.combinations(range(M), 3):
        n = _cross3(V[j] - V[i], V[k] - V[i])
        len2 = _dot3(n, n)
        if not len2 > 0.0:
            continue
        n = n / np.sqrt(len2)
        others = [l for l in range(M) if l not in (i, j, k)]
        dist = _dot3(n[None], V[others] - V[i])
        pos, neg = int((dist > _PLANE_EPS).sum()), int((dist < -_PLANE_EPS).sum())
        near = len(others) - pos - neg
        if pos + neg == 0:
            continue
        nonflat = True
        if pos and neg:
            continue
        if near:
            coplanar = True
        else:
            faces.append((i, j, k))
            normals.append(-n if pos else n)
    if not nonflat:
        raise RuntimeError(f"palette_hull: {_LUT_STATUS_TEXT[_lib.LUT_FLAT]}")
    if coplanar or len(faces) > _lib.LUT_MAX_FACES:
        raise RuntimeError(f"palette_hull: {_LUT_STATUS_TEXT[_lib.LUT_COPLANAR]}")
    if len(faces) < 4:
        raise RuntimeError(f"palette_hull: {_LUT_STATUS_TEXT[_lib.LUT_FLAT]}")
    return order, V, np.array(faces), np.array(normals)


def _closest_on_triangles(p, a, ab, ac):
    """closest point of the triangles (a, a + ab, a + ac) [F,3] to the points p [N,3] -> [N,F,3]: the Voronoi regions in the kernel's order"""
    p = p[:, None, :]
    ap, bp, cp = p - a, p - (a + ab), p - (a + ac)
    d1, d2, d3, d4, d5, d6 = _dot3(ab, ap), _dot3(ac, ap), _dot3(ab, bp), _dot3(ac, bp), _dot3(ab, cp), _dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        total = (va + vb) + vc
        v, w = vb / total, vc / total                                                        # the inside, unless a region below claims the point
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        regions = [((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1.0 - wbc, wbc),            # (the last rule first: an earlier one overwrites it)
                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 0.0, d2 / (d2 - d6)),
                   ((d6 >= 0) & (d5 <= d6), 0.0, 1.0),
                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), 0.0),
                   ((d3 >= 0) & (d4 <= d3), 1.0, 0.0),
                   ((d1 <= 0) & (d2 <= 0), 0.0, 0.0)]
        for mask, rv, rw in regions:
            v, w = np.where(mask, rv, v), np.where(mask, rw, w)
    return a + (v[..., None] * ab + w[..., None] * ac)


def palette_weights_per_op(points, palette, normalize_input=False, return_info=False):
    """pnr_lut_weights' statement in numpy float64 on the host, operation for operation (the hull by brute force, the closest point on every
    triangle, the star tetrahedra's inverse edge matrices): what the device call is measured and tested against.  points [N,3] -> [N,M];
    with return_info also {"outside": [N] bool, "projected": [N,3], "faces", "order"}."""
    order, V, faces, normals = palette_hull(palette)
    x = np.array(points, dtype=np.float64).reshape(-1, 3)
    if normalize_input:
        x = x + 0.05
        x = x / np.sqrt(_dot3(x, x))[:, None]
    a, ab, ac = V[faces[:, 0]], V[faces[:, 1]] - V[faces[:, 0]], V[faces[:, 2]] - V[faces[:, 0]]
    outside = (_dot3(normals, x[:, None, :] - a) > _OUTSIDE_EPS).any(axis=1)
    if outside.any():
        xo = x[outside]
        c = _closest_on_triangles(xo, a, ab, ac)
        e = xo[:, None, :] - c
        x[outside] = c[np.arange(xo.shape[0]), np.argmin(_dot3(e, e), axis=1)]           # argmin: the first of equal minima, the lower face
    star = faces[faces[:, 0] != 0]
    cols = [V[star[:, m]] - V[0] for m in range(3)]                                      # [T,3] each: the columns of the edge matrices
    rows = [_cross3(cols[(m + 1) % 3], cols[(m + 2) % 3]) for m in range(3)]
    det = _dot3(cols[0], rows[0])
    y = (x - V[0])[:, None, :]
    b = [_dot3(rows[m] / det[:, None], y) for m in range(3)]                             # [N,T] each
    b0 = 1.0 - ((b[0] + b[1]) + b[2])
    best = np.argmax(np.minimum(np.minimum(b0, b[0]), np.minimum(b[1], b[2])), axis=1)   # argmax: the first of equal maxima
    n = np.arange(x.shape[0])
    W = np.zeros((x.shape[0], V.shape[0]), dtype=np.float64)
    W[n, order[0]] = b0[n, best]
    for m in range(3):
        W[n, order[star[best, m]]] = b[m][n, best]
    if return_info:
        return W, {"outside": outside, "projected": x, "faces": faces, "order": order}
    return W


def weight_lut_per_op(palette, normalize_input=False):
    """The reference's hist_weights table [32,32,32,M] float64 (palette/utils.py:235-245) by palette_weights_per_op: the host leg the device's
    weight_lut is measured and tested against.  The reference's own loop needs scipy, cvxopt and a Cython module; this needs numpy."""
    W = palette_weights_per_op(bin_centers_of(5).astype(np.float64), palette, normalize_input=normalize_input)
    return W.reshape(32, 32, 32, W.shape[1])


# ---------------------------------------------------------------- the hull simplification (pnr_hull_simplify, include/pnr_hull.h)
_HULL_STATUS_TEXT = {_lib.HULL_COPLANAR: "a supporting plane of a hull carries a fourth point within 1e-9 (the triangulation of that facet is qhull's choice)",
                     _lib.HULL_FLAT: "a point set has no point off the plane of any triple (no hull)",
                     _lib.HULL_DENSE: f"an edge has more than {_lib.HULL_MAX_RELATED} related faces (the compiled cap)"}
_HULL_HEAD = 3 * _lib.HULL_MAX_M + 8 + 4           # float64 words read back by every call: palette | errors | info (8 int32)


def _hull_inputs(centers, center_weights, error_thres, target_size, keep_device=False):
    """(centers [K,3], weights [K], error_thres, target) checked: float64 host arrays, or with keep_device a device tensor as it is."""
    def rows(a, shape):
        if keep_device and torch.is_tensor(a) and a.is_cuda:
            return a.detach().reshape(shape)
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
    c, w = rows(centers, (-1, 3)), rows(center_weights, (-1,))
    if not 4 <= c.shape[0] <= _lib.EXTRACT_MAX_K or w.shape[0] != c.shape[0]:
        raise ValueError(f"simplify_hull: 4..{_lib.EXTRACT_MAX_K} centres [K,3] with their K weights are needed, got {c.shape[0]} and {w.shape[0]}")
    if not float(error_thres) >= 0:
        raise ValueError("simplify_hull: error_thres is negative or NaN")
    target = 0 if target_size is None else int(target_size)
    if target and not 4 <= target <= _lib.HULL_MAX_M:
        raise ValueError(f"simplify_hull: target_size is None or 4..{_lib.HULL_MAX_M}")
    return c, w, float(error_thres), target


def _launch_hull(centers, center_weights, error_thres, target, want_trace=False):
    """ONE launch of pnr_hull_simplify and one read-back of 480 bytes (the set beyond 16 rows and the trace: a second one, only when they are
    needed).  -> {"info": [8] ints, "palette": [16,3], "errors": [8], "vertices": [info[1],3] or None, "trace": [collapses,4] or None}."""
    dev = next((a.device for a in (centers, center_weights) if torch.is_tensor(a) and a.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("simplify_hull needs the HIP path (a CUDA/HIP device); there is no CPU fallback")
        dev = torch.device("cuda")

    def on_device(a, shape):
        t = a.detach() if torch.is_tensor(a) else torch.tensor(np.asarray(a, dtype=np.float64))
        return t.to(dev, torch.float64).reshape(shape).contiguous()
    c, w = on_device(centers, (-1, 3)), on_device(center_weights, (-1,))
    K = c.shape[0]
    out = torch.zeros(_HULL_HEAD + 3 * K + 2 * K, dtype=torch.float64, device=dev)
    base = out.data_ptr()
    a = _lib.HullSimplifyArgs()
    a.centers, a.center_weights, a.K, a.error_thres, a.target_size = c.data_ptr(), w.data_ptr(), K, error_thres, target
    a.palette, a.errors, a.info = base, base + 8 * 3 * _lib.HULL_MAX_M, base + 8 * (3 * _lib.HULL_MAX_M + 8)
    a.vertices, a.trace = base + 8 * _HULL_HEAD, base + 8 * (_HULL_HEAD + 3 * K)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pnr_hull_simplify(ctypes.byref(a), stream_ptr()), "pnr_hull_simplify")
    head = out[:_HULL_HEAD].cpu().numpy()
    info = [int(v) for v in head[3 * _lib.HULL_MAX_M + 8:].view(np.int32)]
    res = {"info": info, "palette": head[:3 * _lib.HULL_MAX_M].reshape(-1, 3).copy(), "errors": head[3 * _lib.HULL_MAX_M:3 * _lib.HULL_MAX_M + 8].copy(),
           "vertices": None, "trace": None}
    if info[0] != _lib.HULL_OK or info[1] > _lib.HULL_MAX_M or want_trace:
        rest = out[_HULL_HEAD:].cpu().numpy()
        res["vertices"] = rest[:3 * info[1]].reshape(-1, 3).copy()
        res["trace"] = rest[3 * K:].view(np.int32).reshape(K, 4)[:info[2]].copy()
    return res


def simplify_hull(centers, center_weights, error_thres=5 / 255, target_size=None, return_info=False):
    """Hull_Simplification_posternerf(centers, prefix, pixel_counts=center_weights, error_thres, target_size) (palette/utils.py:230-234) on the
    device: the convex hull of the K-means centres, one edge collapse after the other -- each the cheapest of the edges' linear programs --
    until the reconstruction error of the centres passes error_thres (or the hull has target_size vertices).  centers [K,3], center_weights
    [K], 4 <= K <= 128, device tensors (extract_centers' without a copy) or host arrays; ONE launch, 480 bytes read back.  Returns the palette
    [M,3] float64 (numpy), with return_info also a dict: status, M, collapses, initial (the first hull's vertices), stop ("error", "target",
    "unchanged", "four"), related (the largest related-face count of an edge), errors {V: error}, trace [(v1, v2, V after, candidates)],
    handed_over (False, or the status text: the kernel met a coplanar facet or an edge above its related-face cap, and the loop was finished
    on the host by simplify_hull_per_op from the vertex set it returned).  A flat set has no hull on the host either: RuntimeError."""
    c, w, thres, target = _hull_inputs(centers, center_weights, error_thres, target_size, keep_device=True)
    raw = _launch_hull(c, w, thres, target, want_trace=bool(return_info))
    status, M, collapses, initial, stop, related = raw["info"][:6]
    errors = {V: (None if raw["errors"][10 - V] == _lib.HULL_ERROR_FAIL else float(raw["errors"][10 - V]))
              for V in range(10, 3, -1) if raw["errors"][10 - V] != _lib.HULL_ERROR_NONE}
    info = {"status": status, "M": M, "collapses": collapses, "initial": initial, "stop": _lib.HULL_STOP[stop], "related": related,
            "errors": errors, "trace": [] if raw["trace"] is None else [tuple(int(v) for v in row) for row in raw["trace"]], "handed_over": False}
    if status == _lib.HULL_FLAT:
        raise RuntimeError(f"pnr_hull_simplify: {_HULL_STATUS_TEXT[status]}")
    if status != _lib.HULL_OK:
        start = raw["vertices"] if raw["vertices"] is not None else raw["palette"][:M]
        palette, rest = simplify_hull_per_op(c, w, thres, target_size, return_info=True, start=start)
        info.update(M=palette.shape[0], collapses=collapses + rest["collapses"], stop=rest["stop"], related=max(related, rest["related"]),
                    errors={**errors, **rest["errors"]}, trace=info["trace"] + rest["trace"], handed_over=_HULL_STATUS_TEXT[status])
        if collapses == 0:
            info["initial"] = rest["initial"]
    else:
        palette = raw["palette"][:M].copy() if M <= _lib.HULL_MAX_M else raw["vertices"]
    return (palette, info) if return_info else palette


def _scipy_hull(points):
    """scipy's hull of a point set as the reference writes it to its OBJ file: (vertices [V,3] in ascending input order, faces [F,3] in the
    vertices' numbering turned outwards)."""
    from scipy.spatial import ConvexHull
    hull = ConvexHull(points)
    verts = np.sort(hull.vertices)
    renum = np.full(points.shape[0], -1)
    renum[verts] = np.arange(verts.shape[0])
    faces = renum[hull.simplices]
    V = hull.points[verts]
    inward = _dot3(_cross3(V[faces[:, 1]] - V[faces[:, 0]], V[faces[:, 2]] - V[faces[:, 0]]), hull.equations[:, :3]) < 0
    faces[inward] = faces[inward][:, [0, 2, 1]]
    return V, faces


def _collapse_per_op(V, faces):
    """remove_one_edge_by_finding_smallest_adding_volume_with_test_conditions(mesh, option=2) (Convexhull_simplification.py:149-322) with
    scipy's HiGHS for cvxopt's GLPK: -> (v1, v2, new point, candidates, largest related-face count), or (None, None, None, 0, largest)."""
    from scipy.optimize import linprog
    edges = sorted({(int(min(u, v)), int(max(u, v))) for f in faces for u, v in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))})
    best, cands, most = None, 0, 0
    for v1, v2 in edges:
        rel = [f for f in faces if v1 in f or v2 in f]
        most = max(most, len(rel))
        A, b, c = [], [], np.zeros(3)
        for f in rel:
            n = np.cross(V[f[1]] - V[f[0]], V[f[2]] - V[f[0]])
            n = n / np.sqrt(np.dot(n, n))
            A.append(n)
            b.append(np.dot(n, V[f[0]]))
            c += n
        res = linprog(c, A_ub=-np.asarray(A), b_ub=-np.asarray(b), bounds=(None, None), method="highs")
        if res.status != 0:
            continue
        cands += 1
        volume = np.asarray([abs(np.dot(np.cross(V[f[1]] - V[f[0]], V[f[2]] - V[f[0]]), res.x - V[f[0]])) / 6.0 for f in rel]).sum()
        if best is None or volume < best[0]:
            best = (volume, v1, v2, res.x)
    if best is None:
        return None, None, None, 0, most
    return best[1], best[2], best[3], cands, most


def _error_per_op(vertices, points, counts):
    """outsidehull_points_distance_unique_data_version (Additive_mixing_layers_extraction.py:185-201); raises what qhull raises."""
    from scipy.spatial import ConvexHull, Delaunay
    hull = ConvexHull(vertices)
    outside = Delaunay(vertices).find_simplex(points, tol=1e-8) < 0
    if not outside.any():
        return 0.0
    tri = hull.points[hull.simplices]
    q = _closest_on_triangles(points[outside], tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    e = points[outside][:, None, :] - q
    dist = np.sqrt(_dot3(e, e)).min(axis=1)
    return float((((dist ** 2) * counts[outside]).sum() / counts.sum()) ** 0.5)


def simplify_hull_per_op(centers, center_weights, error_thres=5 / 255, target_size=None, return_info=False, start=None):
    """Hull_Simplification_posternerf (rgbsg/hull_simplification_posternerf.py:19-77) on the host in its line order, with scipy.spatial.ConvexHull
    and scipy.optimize.linprog(method="highs") where the reference has its OBJ round trip and cvxopt's GLPK (neither imports here): what
    simplify_hull is measured and tested against, and what finishes its hand-overs (start: the vertex set to go on from; the error is always
    taken against the centres).  Returns simplify_hull's results."""
    c, w, thres, target = _hull_inputs(centers, center_weights, error_thres, target_size)
    V, faces = _scipy_hull(c if start is None else np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3))
    info = {"status": _lib.HULL_OK, "collapses": 0, "initial": V.shape[0], "related": 0, "errors": {}, "trace": [], "handed_over": False}

    def done(Vset, stop):
        palette = Vset.clip(0.0, 1.0).reshape(-1, 3)
        info.update(M=palette.shape[0], stop=stop)
        return (palette, info) if return_info else palette

    for _ in range(5000):
        old = V
        v1, v2, x, cands, most = _collapse_per_op(V, faces)
        info["related"] = max(info["related"], most)
        if x is not None:
            keep = [i for i in range(V.shape[0]) if i not in (v1, v2)]
            V, faces = _scipy_hull(np.vstack((V[keep], x)))
            info["collapses"] += 1
            info["trace"].append((v1, v2, V.shape[0], cands))
        n = V.shape[0]
        if n <= 10:
            if not target:
                try:
                    err = _error_per_op(V.clip(0.0, 1.0), c, w)
                except Exception:       # noqa: BLE001 -- the reference's bare except around the same call: qhull refusing the clipped set
                    err = None
                info["errors"][n] = err
                if err is None or err > thres:
                    return done(old, "error")
            elif n == target:
                return done(V, "target")
        if n == old.shape[0] or n == 4:
            return done(V, "unchanged" if n == old.shape[0] else "four")
    raise RuntimeError("simplify_hull_per_op: hull simplification failed")


def save_palette(path, palette):
    """The palette as the reference writes it: a path ending in .npz gets `palette.npz` (key 'palette', float64 [M,3]), any other path
    write_palette_txt's text (rgbsg/hull_simplification_posternerf.py:86-95: "r g b" a line, str() of the float64, no newline after the last
    line).  load_palette reads both back."""
    p = np.asarray(palette.detach().cpu() if torch.is_tensor(palette) else palette, dtype=np.float64).reshape(-1, 3)
    if str(path).endswith(".npz"):
        np.savez(path, palette=p)
    else:
        with open(path, "w") as f:
            f.write("\n".join(f"{c[0]} {c[1]} {c[2]}" for c in p))


def extract_palette(model, poses, intrinsics, H, W, images, palette_model=None, palette_size=None, error_thres=5 / 255, normalize_input=False, **kw):
    """The whole of step 2 (PaletteTrainer.extract_palette into palette_extraction, palette/utils.py:167-254): extract_centers ->
    simplify_hull -> the weight LUT, which with a `palette_model` is handed to it (initialize_from_extraction) and otherwise built on the
    NeRF model's device (weight_lut).  kw: extract_centers' (linear, thresh, tau, frames_in_flight, render arguments).  Returns (palette [M,3]
    float64, the LUT float32 [1,M,32,32,32] on the device, extract_centers' result).  The reference's OBJ files and extract-palette.png are not
    written; save_palette and save_lut write its palette and hist_weights files."""
    res = extract_centers(model, poses, intrinsics, H, W, images, **kw)
    palette = simplify_hull(res["centers"], res["center_weights"], error_thres=error_thres, target_size=palette_size)
    if palette_model is not None:
        lut = initialize_from_extraction(palette_model, palette, normalize_input=normalize_input)
    else:
        lut = weight_lut(palette, normalize_input=normalize_input, device=next(model.parameters()).device)
    return palette, lut, res
