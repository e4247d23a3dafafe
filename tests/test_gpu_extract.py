"""pnr_extract_accumulate and pnr_extract_kmeans on the device, and the loops over them (palettenerf_amd.extract), against the float64 statement of
tests/extract_reference.py.

Accumulate.  The valid total is exact.  A table may differ from the statement's only where a sample sits on a fence: with B = the valid samples
whose float64 colour lies within 2^-20 of a bin boundary of that grid, the L1 distance of the tables is at most 2 B (a sample that moves to the
neighbouring bin changes two counts by one).  Every input must have B <= 0.1 % of its valid samples -- asserted, so that a bad input cannot hide a
failure; for the shapes below B is 0 or 1.  Shapes: N = 1, 63, 257, 1000 (ragged ends of a wave, of a workgroup), and the smallest N at which a
workgroup takes a second trip of its grid-stride loop, from pnr_launch_geometry.

k-means.  Labels, the iteration count and the stop rule equal the statement's; centres and weights are float64 sums of at most P terms in another
order, so they agree within P 2^-52 relative; two runs give the same bits.

End to end.  extract_centers against extract_centers_per_op (the reference's own sequence, with the float64 host k-means: scikit-learn's float32
run is tied to the statement in tests/test_extract_host.py) on images chosen so that NO pixel of theirs is on a fence (B = 0 for any mask):
the tables are then equal and the centres agree within the k-means bound (matched by centre where two weights tie: same_clusters)."""
import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, extract, scene, trainset
from palettenerf_amd import rays as prays
from tests import extract_reference as ref
from tests.test_gpu_jitter import make_model

pytestmark = pytest.mark.gpu

KW = dict(max_steps=1024, T_thresh=1e-4)
NP_DTYPE = {"fp32": np.float32, "fp16": np.float16, "uint8": np.uint8}


# ---------------------------------------------------------------- accumulate
def make_view(seed, H, W, C, storage):
    """(weights_sum [H W] float32, view [H,W,C] as stored): colours uniform in [0, 1], weights uniform in [0, 1] with exact 0.5s and NaNs mixed in"""
    rng = np.random.default_rng(seed)
    n = H * W
    ws = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if n >= 8:
        special = rng.choice(n, size=max(2, n // 16), replace=False)
        ws[special[::2]] = np.float32(0.5)
        ws[special[1::2]] = np.float32("nan")
    if storage == "uint8":
        view = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    else:
        view = rng.uniform(0.0, 1.0, size=(H, W, C)).astype(NP_DTYPE[storage])
    return ws, view


def device_tables(hist):
    buf = hist._buf.cpu().numpy()
    return buf[:512].copy(), buf[512:512 + 32768].copy(), int(buf[-1])


def check_tables(got, want, what):
    """got = (coarse, fine, total) of the device, want = the statement's dict (or a sum of them)"""
    coarse, fine, total = got
    l1_fine, l1_coarse = int(np.abs(fine - want["fine"]).sum()), int(np.abs(coarse - want["coarse"]).sum())
    print(f"{what}: valid {want['total']}  B5 {want['B5']} L1 {l1_fine}  B3 {want['B3']} L1 {l1_coarse}")
    assert max(want["B5"], want["B3"]) <= 1e-3 * want["total"], f"{what}: the input has too many samples on a fence"
    assert total == want["total"], what
    assert int(fine.sum()) == total and int(coarse.sum()) == total, what
    assert l1_fine <= 2 * want["B5"] and l1_coarse <= 2 * want["B3"], what


def accumulate_once(cuda, ws, view, linear=False, thresh=0.5, hist=None):
    hist = extract.RadianceHistogram(cuda) if hist is None else hist
    hist.update(torch.from_numpy(ws).to(cuda), torch.from_numpy(view).to(cuda), linear=linear, thresh=thresh)
    return hist


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("storage", ["fp32", "fp16", "uint8"])
def test_accumulate_equals_the_statement_for_every_storage_and_ragged_sizes(cuda, storage, C):
    for N, (H, W) in ((1, (1, 1)), (63, (7, 9)), (257, (1, 257)), (1000, (25, 40))):
        seed = 100 * N + C
        while any(max(a["B3"], a["B5"]) > 1e-3 * a["total"] for a in (ref.accumulate(*make_view(seed, H, W, C, storage), linear=lin) for lin in (False, True))):
            seed += 10000                                                           # (at these sizes one sample on a fence is too many: the next seed)
        for linear in (False, True):
            ws, view = make_view(seed, H, W, C, storage)
            want = ref.accumulate(ws, view, linear=linear)
            if N > 1:
                assert 0 < want["total"] < N
            hist = accumulate_once(cuda, ws, view, linear=linear)
            got = device_tables(hist)
            check_tables(got, want, f"{storage} C {C} N {N} linear {linear}")
            again = device_tables(accumulate_once(cuda, ws, view, linear=linear))
            assert all(np.array_equal(a, b) for a, b in zip(got[:2], again[:2])) and got[2] == again[2]       # two runs: identical tables


@pytest.mark.parametrize("storage,C,shape", [("fp32", 3, "flat"), ("uint8", 4, "rows")])
def test_accumulate_on_a_second_trip_of_the_grid_stride_loop(cuda, storage, C, shape):
    wg, per_trip = _lib.launch_geometry("pnr_extract_accumulate", 1 << 40)        # the capped grid
    N = wg * per_trip + 1                                                          # the smallest view with a pixel on a second trip
    assert _lib.launch_geometry("pnr_extract_accumulate", N) == (wg, per_trip) and _lib.launch_geometry("pnr_extract_accumulate", N - 1) == (wg, per_trip)
    assert _lib.launch_geometry("pnr_extract_accumulate", N - 1 - per_trip) == (wg - 1, per_trip)
    H, W = (1, N) if shape == "flat" else (5, N // 5)
    assert H * W == N
    ws, view = make_view(7, H, W, C, storage)
    ws[-1] = 0.75                                                                   # the one pixel of the second trip counts
    want = ref.accumulate(ws, view)
    check_tables(device_tables(accumulate_once(cuda, ws, view)), want, f"second trip {storage} C {C} N {N}")
    ws[-1] = 0.25
    without = ref.accumulate(ws, view)
    assert without["total"] == want["total"] - 1


def test_accumulate_reads_padded_rows_and_unaligned_bases(cuda):
    H, W = 19, 23
    for storage, C, pad, lead in (("fp32", 3, 5, 0), ("uint8", 3, 3, 1), ("fp16", 4, 2, 0), ("uint8", 4, 1, 0), ("fp32", 4, 0, 1), ("fp16", 4, 0, 3)):
        ws, view = make_view(31 + C, H, W, C, storage)
        want = ref.accumulate(ws, view)
        # the view as columns [0, W) of rows W + pad pixels long, `lead` scalar elements behind an aligned base
        flat = torch.zeros(lead + H * (W + pad) * C + 8, dtype=torch.from_numpy(view).dtype, device=cuda)
        if flat.dtype != torch.uint8:
            flat.fill_(0.77)                                                        # what the padding holds must not matter
        rows = flat[lead:lead + H * (W + pad) * C].view(H, W + pad, C)
        rows[:, :W] = torch.from_numpy(view).to(cuda)
        padded = rows[:, :W]
        assert padded.stride(0) == (W + pad) * C and (pad == 0 or not padded.is_contiguous())
        hist = extract.RadianceHistogram(cuda).update(torch.from_numpy(ws).to(cuda), padded)
        check_tables(device_tables(hist), want, f"padded {storage} C {C} pad {pad} lead {lead}")


def test_accumulate_adds_to_what_the_tables_hold(cuda):
    views = [make_view(50 + i, 12, 17, 4, st) for i, st in enumerate(("fp32", "fp16", "uint8"))]
    wants = [ref.accumulate(ws, v) for ws, v in views]
    singles = [device_tables(accumulate_once(cuda, ws, v)) for ws, v in views]
    hist = extract.RadianceHistogram(cuda)
    for ws, v in views:
        accumulate_once(cuda, ws, v, hist=hist)
    coarse, fine, total = device_tables(hist)
    assert np.array_equal(coarse, sum(s[0] for s in singles)) and np.array_equal(fine, sum(s[1] for s in singles)) and total == sum(s[2] for s in singles)
    both = {k: sum(w[k] for w in wants) for k in ("coarse", "fine", "total", "B3", "B5")}
    check_tables((coarse, fine, total), both, "three views")
    assert hist.total == total and hist.counts(5).dtype == torch.int64 and tuple(hist.counts(3).shape) == (512,)
    bw, bc = hist.bin_weights(5), hist.bin_centers(5)
    assert bw.dtype == torch.float64 and tuple(bw.shape) == (32768,) and bc.dtype == torch.float32 and tuple(bc.shape) == (32768, 3)
    assert np.array_equal(bw.cpu().numpy(), fine.astype(np.float64)) and np.array_equal(bc.cpu().numpy().astype(np.float64), ref.bin_centers(5))
    # a view with nothing valid -- weights at most 0.5, or NaN -- leaves the tables as they are
    ws = np.full(12 * 17, 0.5, dtype=np.float32)
    ws[::3] = np.float32("nan")
    ws[1::3] = 0.0
    accumulate_once(cuda, ws, views[0][1], hist=hist)
    after = device_tables(hist)
    assert np.array_equal(after[0], coarse) and np.array_equal(after[1], fine) and after[2] == total
    hist.clear()
    assert hist.total == 0 and int(hist.counts(5).sum()) == 0 and int(hist.counts(3).sum()) == 0


def test_accumulate_excludes_one_half_and_nan_and_obeys_the_threshold(cuda):
    ws = np.array([0.5, np.nan, np.nextafter(np.float32(0.5), np.float32(1)), 0.4999, 1.0, np.inf, -np.inf, 0.0], dtype=np.float32)
    view = np.random.default_rng(3).uniform(0, 1, size=(1, 8, 3)).astype(np.float32)
    want = ref.accumulate(ws, view)
    assert want["total"] == 3
    check_tables(device_tables(accumulate_once(cuda, ws, view)), want, "0.5 and NaN")
    want = ref.accumulate(ws, view, thresh=0.25)
    assert want["total"] == 5
    check_tables(device_tables(accumulate_once(cuda, ws, view, thresh=0.25)), want, "thresh 0.25")


@pytest.mark.parametrize("storage", ["fp32", "uint8"])
@pytest.mark.parametrize("level", [0, 1])
def test_accumulate_of_an_all_black_and_an_all_white_view(cuda, storage, level):
    H, W = 9, 14
    view = np.full((H, W, 3), level * (255 if storage == "uint8" else 1), dtype=NP_DTYPE[storage])
    ws = np.ones(H * W, dtype=np.float32)
    for linear in (False, True):
        want = ref.accumulate(ws, view, linear=linear)
        assert want["total"] == H * W and int((want["fine"] > 0).sum()) == 1 and want["B5"] == 0        # one bin: (1, 1, 1) / sqrt(3), off every fence
        check_tables(device_tables(accumulate_once(cuda, ws, view, linear=linear)), want, f"level {level} {storage} linear {linear}")


# ---------------------------------------------------------------- k-means
def run_kmeans(cuda, coarse, fine, total, tau, max_iter=300, tol=1e-4):
    hist = extract.RadianceHistogram(cuda).load_counts(coarse, fine, total)
    return extract.kmeans_centers(hist, tau=tau, max_iter=max_iter, tol=tol, return_labels=True)


def check_kmeans(cuda, coarse, fine, total, tau, max_iter=300, what=""):
    X, w, init = ref.points_of(coarse, fine, total, tau)
    want = ref.run_kmeans(X, w, init, max_iter=max_iter)
    c, cw, info = run_kmeans(cuda, coarse, fine, total, tau, max_iter)
    P, K = X.shape[0], init.shape[0]
    assert (info["K"], info["P"]) == (K, P), what
    assert np.array_equal(info["labels"], want["labels"]), what
    assert info["iterations"] == want["iterations"] and info["stop"] == want["stop"], (what, info["iterations"], info["stop"], want["iterations"], want["stop"])
    bound = P * 2.0 ** -52
    err_c = float((np.abs(c - want["sorted_centers"]) / np.abs(want["sorted_centers"])).max())
    nz = want["center_weights"] > 0
    err_w = float((np.abs(cw - want["center_weights"])[nz] / want["center_weights"][nz]).max()) if nz.any() else 0.0
    print(f"{what} P {P} K {K} max_iter {max_iter}: iterations {info['iterations']} stop {info['stop']} emptied {info['emptied']}  "
          f"centres {err_c:.3g} weights {err_w:.3g} bound {bound:.3g}")
    assert c.shape == (K, 3) and cw.shape == (K,) and c.dtype == np.float64 and cw.dtype == np.float64
    assert err_c <= bound and err_w <= bound and np.array_equal(cw[~nz], want["center_weights"][~nz]), what
    c2, cw2, info2 = run_kmeans(cuda, coarse, fine, total, tau, max_iter)
    assert c.tobytes() == c2.tobytes() and cw.tobytes() == cw2.tobytes() and np.array_equal(info["labels"], info2["labels"]), what     # the same bits
    return want, info


# (P, K, seed, max_iter, the stop rule the statement ends by)
KMEANS_CASES = [(1, 1, 0, 300, "labels"), (7, 7, 0, 300, "labels"), (37, 3, 0, 300, "shift"), (37, 3, 1, 300, "labels"), (5000, 40, 52, 300, "shift"),
                (2000, 124, 0, 300, "shift"), (37, 3, 0, 1, "max_iter"), (37, 3, 0, 2, "max_iter"), (5000, 40, 52, 1, "max_iter"),
                (5000, 40, 52, 2, "max_iter")]


@pytest.mark.parametrize("P,K,seed,max_iter,stop", KMEANS_CASES)
def test_kmeans_equals_the_statement(cuda, P, K, seed, max_iter, stop):
    coarse, fine, total, tau = ref.seeded_tables(seed, P, K)
    want, info = check_kmeans(cuda, coarse, fine, total, tau, max_iter, f"seed {seed}")
    assert want["stop"] == stop and not want["emptied"] and info["emptied"] is False


def test_kmeans_tie_goes_to_the_lower_index(cuda):
    """Centres (2, 6, 2) / 32 and (6, 2, 2) / 32 -- coarse bins (0, 1, 0) and (1, 0, 0) -- and the point (3.5, 3.5, 0.5) / 32, equidistant from both in
    exact and in float64 arithmetic; one point on either side.  With max_iter = 1 the centres after iteration 0 come out: the tied point has to be
    in the first cluster's mean."""
    fine, coarse = np.zeros(32768, dtype=np.int64), np.zeros(512, dtype=np.int64)
    fine[(1 << 10) | (5 << 5)], fine[(3 << 10) | (3 << 5)], fine[(5 << 10) | (1 << 5)] = 30, 50, 30
    coarse[1 << 3], coarse[1 << 6] = 55, 55
    X, w, init = ref.points_of(coarse, fine, 110, 0.1)
    d = ((X[1] - init) ** 2)
    assert ((d[0, 0] + d[0, 1]) + d[0, 2]) == ((d[1, 0] + d[1, 1]) + d[1, 2])
    want, info = check_kmeans(cuda, coarse, fine, 110, 0.1, max_iter=1, what="tie")
    assert want["labels"].tolist() == [0, 0, 1] and np.abs(want["center_weights"] - np.array([80 / 110, 30 / 110])).max() < 1e-15
    c, cw, _ = run_kmeans(cuda, coarse, fine, 110, 0.1, max_iter=1)
    assert np.abs(cw - np.array([80 / 110, 30 / 110])).max() < 1e-15 and abs(c[0, 0] - 2.75 / 32) < 1e-15 and abs(c[0, 1] - 4.25 / 32) < 1e-15


def test_kmeans_equal_weights_keep_the_cluster_order(cuda):
    """seven points with the same count, one cluster each: every weight is 1/7, and the sort must leave the clusters in index order"""
    coarse, fine, total, _ = ref.seeded_tables(0, 7, 7)
    fine[fine > 0] = 5
    coarse[coarse > 0] = 5
    want, info = check_kmeans(cuda, coarse, fine, 35, 0.1, what="equal weights")
    assert want["order"].tolist() == list(range(7)) and len(set(want["center_weights"].tolist())) == 1
    c, cw, _ = run_kmeans(cuda, coarse, fine, 35, 0.1)
    assert np.abs(c - ref.points_of(coarse, fine, 35, 0.1)[0]).max() < 1e-15     # each centre is its point, in ascending code order


def test_kmeans_hands_an_emptied_cluster_to_the_host(cuda):
    coarse, fine, total, tau = ref.emptied_tables()
    want = ref.run_kmeans(*ref.points_of(coarse, fine, total, tau))
    assert want["emptied"] == [1]
    c, cw, info = run_kmeans(cuda, coarse, fine, total, tau)
    assert info["emptied"] == 1, "the device stops in the iteration that empties the cluster and says so"
    assert info["iterations"] == want["iterations"] and info["stop"] == want["stop"] and np.array_equal(info["labels"], want["labels"])
    bound = 6 * 2.0 ** -52
    assert (np.abs(c - want["sorted_centers"]) <= bound * np.abs(want["sorted_centers"])).all()
    assert (np.abs(cw - want["center_weights"]) <= bound * want["center_weights"]).all()


def test_kmeans_refuses_what_it_cannot_cluster(cuda):
    coarse, fine, total, tau = ref.seeded_tables(0, 37, 3)
    with pytest.raises(RuntimeError, match="K = 0"):
        run_kmeans(cuda, coarse, fine, total, 0.9999)
    few = np.zeros(512, dtype=np.int64)
    few[:9] = 100
    with pytest.raises(RuntimeError, match="P < K"):
        run_kmeans(cuda, few, (np.arange(32768) < 5).astype(np.int64), 900, 1e-3)
    with pytest.raises(RuntimeError, match="compiled cap"):
        run_kmeans(cuda, np.full(512, 2, dtype=np.int64), np.ones(32768, dtype=np.int64), 1024, 1e-3 / 2)


# ---------------------------------------------------------------- end to end
def fence_free_images(n, H, W, storage, first_seed):
    """[n,H,W,4] images none of whose pixels is within the fence of a boundary of either grid (B = 0 whatever the mask): the first seed that gives one"""
    for seed in range(first_seed, first_seed + 64):
        rng = np.random.default_rng(seed)
        img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8) if storage == "uint8" else rng.uniform(0, 1, size=(n, H, W, 4)).astype(np.float32)
        a = ref.accumulate(np.ones(n * H * W, dtype=np.float32), img.reshape(-1, 4))
        if a["B3"] == 0 and a["B5"] == 0:
            return img
    raise AssertionError("no fence-free image among 64 seeds")


def same_clusters(c, cw, c_ref, cw_ref, bound):
    """The same (centre, weight) pairs within `bound` relative, and the same descending weight sequence.  With a few hundred samples two clusters
    often hold the SAME number of samples: their weights are equal in exact arithmetic and differ by a rounding in float64, differently for
    every summation order, so which of the two comes first is not defined by the statement either (its argsort sees the rounding).  The pairs
    are therefore matched by centre, not by position; the positions are held through the weight sequence."""
    assert np.all(np.diff(cw) <= 0)
    assert (np.abs(cw - cw_ref) <= bound * cw_ref).all()
    a, b = np.lexsort(c.T[::-1]), np.lexsort(c_ref.T[::-1])
    assert (np.abs(c[a] - c_ref[b]) <= bound * np.abs(c_ref[b])).all()
    assert (np.abs(cw[a] - cw_ref[b]) <= bound * cw_ref[b]).all()


@pytest.mark.parametrize("storage", ["fp32", "uint8"])
@pytest.mark.parametrize("H,W", [(16, 16), (33, 17)])
@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_extract_centers_equals_the_per_op_sequence(cuda, tmp_path, kind, H, W, storage):
    m = make_model(kind, cuda, 0, 100.0)
    intr = scene.intrinsics_from_fov(H, W)
    poses = np.stack([scene.lookat_pose(azimuth_deg=30.0 + 40.0 * i) for i in range(3)])
    img = fence_free_images(3, H, W, storage, 11)
    if storage == "uint8":
        images = trainset.TrainSet(img, poses, intr, H, W, num_rays=64, storage="uint8", device=cuda)
        assert images.images.dtype == torch.uint8
    else:
        images = torch.from_numpy(img)                                             # a host stack
    tau = 0.02
    res = extract.extract_centers(m, poses, intr, H, W, images, tau=tau, **KW)
    per_op = extract.extract_centers_per_op(m, poses, intr, H, W, images, tau=tau, kmeans="host", **KW)
    # the mask is mixed, and the statement on the frames' own weights_sum gives the same tables
    want = {k: 0 for k in ("coarse", "fine", "total", "B3", "B5")}
    with torch.no_grad():
        for i in range(3):
            ro, rd = prays.rays_from_indices(torch.from_numpy(poses[i:i + 1]).to(cuda), intr, H, W, None)
            r = m.render(ro, rd, bg_color=None, perturb=False, **({"gui_mode": True} if kind == "palette" else {}), **KW)
            a = ref.accumulate(r["weights_sum"].reshape(-1).cpu().numpy(), img[i])
            want = {k: want[k] + a[k] for k in want}
    print(f"{kind} {H}x{W} {storage}: valid {want['total']} of {3 * H * W}, K {res['info']['K']} P {res['info']['P']} iterations {res['info']['iterations']}"
          f" stop {res['info']['stop']} emptied {res['info']['emptied']}")
    assert 0 < want["total"] < 3 * H * W, "the mask must be mixed"
    assert want["B3"] == 0 and want["B5"] == 0
    assert res["total"] == per_op["total"] == want["total"]
    for key, name in (("hist_coarse", "coarse"), ("hist_fine", "fine")):
        assert np.array_equal(res[key], per_op[key]) and np.array_equal(res[key], want[name] / want["total"]), key
    assert np.array_equal(res["hist_rgb"], per_op["hist_rgb"]) and res["hist_rgb"].dtype == np.float32 and res["hist_rgb"].shape == (32768, 3)
    P, K = res["info"]["P"], res["info"]["K"]
    assert (per_op["info"]["P"], per_op["info"]["K"]) == (P, K) and K >= 2
    stmt = ref.run_kmeans(*ref.points_of(want["coarse"], want["fine"], want["total"], tau))
    bound = P * 2.0 ** -52
    for c, cw in ((per_op["centers"], per_op["center_weights"]), (stmt["sorted_centers"], stmt["center_weights"])):
        same_clusters(res["centers"], res["center_weights"], c, cw, bound)
    assert res["info"]["iterations"] == stmt["iterations"] == per_op["info"]["iterations"] and res["info"]["stop"] == stmt["stop"]
    # one .npz, there and back
    path = str(tmp_path / "centers.npz")
    extract.save_centers(path, res)
    back = extract.load_centers(path)
    assert back["total"] == res["total"] and all(np.array_equal(back[k], res[k]) and back[k].dtype == res[k].dtype for k in
                                                  ("centers", "center_weights", "hist_coarse", "hist_fine", "hist_rgb"))
    # two frames in flight: the same tables
    one = extract.radiance_histograms(m, poses, intr, H, W, images, **KW)
    two = extract.radiance_histograms(m, poses, intr, H, W, images, frames_in_flight=2, **KW)
    assert torch.equal(one._buf, two._buf) and one.total == want["total"]


def test_the_sklearn_leg_of_the_per_op_sequence_runs(cuda):
    pytest.importorskip("sklearn")
    H, W = 16, 16
    m = make_model("nerf", cuda, 0, 100.0)
    intr = scene.intrinsics_from_fov(H, W)
    poses = np.stack([scene.lookat_pose(azimuth_deg=30.0 + 40.0 * i) for i in range(3)])
    images = torch.from_numpy(fence_free_images(3, H, W, "fp32", 11))
    res = extract.extract_centers(m, poses, intr, H, W, images, tau=0.02, **KW)
    per_op = extract.extract_centers_per_op(m, poses, intr, H, W, images, tau=0.02, **KW)
    assert per_op["info"]["stop"] is None and per_op["centers"].shape == res["centers"].shape
    print("device - sklearn(float32) centres:", float(np.abs(per_op["centers"] - res["centers"]).max()))
    assert np.array_equal(per_op["hist_fine"], res["hist_fine"]) and per_op["total"] == res["total"]
