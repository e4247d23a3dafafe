"""The palette extraction's k-means on the host, no GPU.

1. The statement (tests/extract_reference.py) against scikit-learn.  The reference calls KMeans on float32 points (bin_centers_fine is float32), so
   scikit-learn's own float32 error is the yardstick: E = the largest centre difference between KMeans on the float32 points and KMeans on the same
   points as float64, and the statement has to agree with the float32 run within 4 E (the project's 4x rule).  E is measured in the test; on
   scikit-learn 1.7.2 it was (the last digit moves between runs: scikit-learn sums in threads)
       P =   40, K =  3, seed  0:  E = 4.24e-08        P = 1500, K = 20, seed  4:  E = 1.07e-07
       P =  300, K =  7, seed  0:  E = 8.53e-08        P = 5000, K = 40, seed 52:  E = 5.59e-06
   so the bound 4 E is 1.7e-07 ... 2.2e-05; the statement differed from the float32 run by E itself and from the float64 run by at most 1.1e-15.  The points lie on a lattice,
   so exact ties between centres happen and rounding decides them: the seeds are those for which scikit-learn's two runs give equal labels (of seeds
   0 .. 59: all for the two small shapes, 14 for P = 1500, 2 for P = 5000), and the test checks that condition first.
2. The product's host routine (extract.lloyd_host, sort_centers, points_of) against the statement to 1e-12, an emptied cluster included."""
import warnings

import numpy as np
import pytest

from palettenerf_amd import extract
from tests import extract_reference as ref

SKLEARN_CASES = [(40, 3, 0), (300, 7, 0), (1500, 20, 4), (5000, 40, 52)]


@pytest.mark.parametrize("P,K,seed", SKLEARN_CASES)
def test_statement_agrees_with_scikit_learn_within_its_own_float32_error(P, K, seed):
    cluster = pytest.importorskip("sklearn.cluster")
    coarse, fine, total, tau = ref.seeded_tables(seed, P, K)
    assert fine.min() >= 0 and fine[fine > 0].min() >= 1 and fine.max() <= 10 ** 7
    X, w, init = ref.points_of(coarse, fine, total, tau)
    assert X.shape == (P, 3) and init.shape == (K, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k32 = cluster.KMeans(n_clusters=K, init=init.astype(np.float32)).fit(X=X.astype(np.float32), sample_weight=w)       # as the reference calls it
        k64 = cluster.KMeans(n_clusters=K, init=init).fit(X=X, sample_weight=w)
    assert np.array_equal(k32.labels_, k64.labels_), "the seed must be one for which scikit-learn's own two runs agree"
    E = float(np.abs(k32.cluster_centers_.astype(np.float64) - k64.cluster_centers_).max())
    r = ref.lloyd(X, w, init)
    err = float(np.abs(r["centers"] - k32.cluster_centers_).max())
    print(f"P {P} K {K} seed {seed}: E {E:.3g}  statement - sklearn(float32) {err:.3g}  - sklearn(float64) {np.abs(r['centers'] - k64.cluster_centers_).max():.3g}"
          f"  iterations {r['iterations']} / {k32.n_iter_} / {k64.n_iter_}  stop {r['stop']}")
    assert E > 0 and not r["emptied"]
    assert np.array_equal(r["labels"], k32.labels_)
    assert err <= 4 * E


@pytest.mark.parametrize("max_iter", [1, 2, 300])
@pytest.mark.parametrize("P,K,seed", SKLEARN_CASES + [(1, 1, 0), (7, 7, 0), (37, 3, 0), (2000, 124, 0)])
def test_host_routine_equals_the_statement(P, K, seed, max_iter):
    coarse, fine, total, tau = ref.seeded_tables(seed, P, K)
    X, w, init = extract.points_of(coarse, fine, total, tau)
    Xr, wr, initr = ref.points_of(coarse, fine, total, tau)
    assert np.array_equal(X, Xr) and np.array_equal(w, wr) and np.array_equal(init, initr)
    r = ref.run_kmeans(Xr, wr, initr, max_iter=max_iter)
    c, labels, n, stop = extract.lloyd_host(X, w, init, max_iter=max_iter)
    assert np.array_equal(labels, r["labels"]) and n == r["iterations"] and stop == r["stop"]
    assert np.abs(c - r["centers"]).max() <= 1e-12
    sc, cw = extract.sort_centers(c, labels, w)
    assert np.abs(sc - r["sorted_centers"]).max() <= 1e-12 and np.abs(cw - r["center_weights"]).max() <= 1e-12
    assert np.all(np.diff(cw) <= 0)


def test_host_routine_relocates_an_emptied_cluster_as_the_statement_does():
    coarse, fine, total, tau = ref.emptied_tables()
    X, w, init = extract.points_of(coarse, fine, total, tau)
    assert X.shape == (6, 3) and init.shape == (3, 3)
    r = ref.run_kmeans(*ref.points_of(coarse, fine, total, tau))
    assert r["emptied"] == [1], "the case is built so that the middle cluster empties in iteration 1"
    c, labels, n, stop = extract.lloyd_host(X, w, init)
    assert np.array_equal(labels, r["labels"]) and n == r["iterations"] and stop == r["stop"]
    assert np.abs(c - r["centers"]).max() <= 1e-12
    assert len(set(labels.tolist())) == 3                      # the relocated cluster has a point again
    # a continuation from the centres the emptied iteration started from -- what pnr_extract_kmeans hands over -- ends in the same place
    first = ref.lloyd(X, w, init, max_iter=1)
    c2, labels2, n2, stop2 = extract.lloyd_host(X, w, first["centers"], max_iter=300 - 1)
    assert np.array_equal(labels2, r["labels"]) and 1 + n2 == r["iterations"] and stop2 == r["stop"]
    assert np.abs(c2 - r["centers"]).max() <= 1e-12


def test_sort_ties_go_to_the_lower_cluster_index():
    centers = np.arange(12, dtype=np.float64).reshape(4, 3)
    labels = np.array([0, 1, 2, 3, 3])
    w = np.array([0.25, 0.125, 0.25, 0.125, 0.125])
    sc, cw = extract.sort_centers(centers, labels, w)
    assert cw.tolist() == [0.25, 0.25, 0.25, 0.125] and np.array_equal(sc, centers[[0, 2, 3, 1]])


def test_bin_centers_are_the_reference_s():
    for bits in (3, 5):
        c = extract.bin_centers_of(bits)
        assert c.dtype == np.float32 and c.shape == (1 << (3 * bits), 3)
        assert np.array_equal(c.astype(np.float64), ref.bin_centers(bits))
    assert extract.bin_centers_of(5)[(3 << 10) | (7 << 5) | 31].tolist() == [3.5 / 32, 7.5 / 32, 31.5 / 32]
