"""The hull simplification on the host (no GPU): the closed statement of tests/hull_reference.py in np.longdouble (the truth) against the chain
that follows the reference's lines with scipy (extract.simplify_hull_per_op: ConvexHull, linprog(method="highs")) on the whole trace of every
fixture; the fixtures' margins; E, the yardstick tests/test_gpu_hull.py holds the kernel to; the palette files; simplify_hull without a device
and its hand-over path with the status injected by a stub.

E is ONE figure: the largest absolute difference between the host formulation's and the truth's palette over all fixtures that have a truth.
As measured: 1.96e-15 (shell-11; profiles/hull/README.md).

Two of the recipes, mix(4, 40) and mix(8, 40), put four or more of the clipped centres EXACTLY on one side plane of the cube (.clip(.02, .98)),
four of them hull vertices: a coplanar facet, which the statement refuses (PNR_HULL_COPLANAR) rather than triangulates.  They stay as cases and
are the natural hand-over: the truth's answer for them is the refusal with the centres returned, and the palette is the host chain's, whose
initial hull and returned size are the recorded 21 / 8 and 18 / 8.  The coplanar points are off their plane by less than 1e-15, a million times
below the 1e-9 rule, so this decision does not rest on rounding either."""
import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, extract
from tests import hull_reference as ref

names = pytest.mark.parametrize("name", ref.NAMES)
REFUSED = ("mix-4-40", "mix-8-40")


@names
def test_the_truth_and_the_host_formulation_agree_on_the_whole_trace(name):
    ref.require_longdouble()
    t = ref.truth(name)
    palette, info = ref.host(name)
    initial, returned = ref.EXPECTED[name]
    assert info["initial"] == initial and (returned is None or palette.shape[0] == returned)        # what the issue recorded
    if name in REFUSED:
        c, _ = ref.fixture(name)
        assert t["status"] == ref.COPLANAR and t["collapses"] == 0 and t["M"] == c.shape[0] and np.array_equal(t["palette"].astype(np.float64), c)
        on_side = [int(np.sum(c[:, ax] == v)) for ax in range(3) for v in (.02, .98)]
        assert max(on_side) >= 4                                     # the exact coincidence the recipe's clip makes
        return
    assert t["status"] == ref.OK
    assert t["trace"] == info["trace"], "another edge or another vertex count at some collapse"
    assert (t["initial"], t["collapses"], _lib.HULL_STOP[t["stop"]], t["related"], t["M"]) == \
           (info["initial"], info["collapses"], info["stop"], info["related"], info["M"])
    assert list(t["errors"]) == list(info["errors"])
    for V, e in t["errors"].items():
        assert (e is None) == (info["errors"][V] is None) and (e is None or abs(e - info["errors"][V]) < 1e-12), V
    assert palette.shape == t["palette"].shape and palette.dtype == np.float64
    d = float(np.max(np.abs(palette - t["palette"])))
    print(f"{name}: initial {t['initial']}, returned {t['M']}, collapses {t['collapses']}, related {t['related']}, stop {info['stop']}, "
          f"errors {t['errors']}, host - truth {d:.3e}")
    assert d < 1e-12
    assert palette.min() >= 0 and palette.max() <= 1


@names
def test_the_fixture_margins_hold(name):
    t = ref.truth(name)
    if name in REFUSED:
        assert t["plane_margin"] > 0.99e-9          # the coplanar points are ON their plane: the whole 1e-9 of the rule away from its threshold
        return
    print(f"{name}: plane margin {t['plane_margin']:.3e}, smallest relative cost gap {t['cost_gap']:.3e}, error margin {t['error_margin']:.3e}")
    assert t["plane_margin"] >= ref.MIN_PLANE_MARGIN
    assert t["cost_gap"] >= ref.MIN_COST_GAP
    assert t["error_margin"] >= ref.MIN_ERROR_MARGIN


def test_the_recorded_figures_of_the_fixtures():
    t = ref.truth("mix-1-24")
    assert [round(t["errors"][V], 4) for V in (10, 9, 8)] == [0.0078, 0.0181, 0.0297] and abs(t["cost_gap"] - 5.3e-2) < 1e-3
    t = ref.truth("mix-2-44")
    assert round(t["errors"][6], 4) == 0.0130 and round(t["errors"][5], 4) == 0.0218 and max(t["errors"][V] for V in (10, 9, 8, 7, 6)) < 5 / 255
    t = ref.truth("shell-11")
    assert (t["initial"], t["M"], t["collapses"], t["related"]) == (55, 7, 49, 18)
    assert round(t["errors"][7], 4) == 0.0149 and round(t["errors"][6], 4) == 0.0317 and abs(t["cost_gap"] - 4.5e-3) < 1e-4
    for name in ("tiny-20-4", "tiny-21-5"):         # every LP is infeasible: the input hull comes back
        t, (c, _) = ref.truth(name), ref.fixture(name)
        assert t["collapses"] == 0 and t["stop"] == ref.STOP_UNCHANGED and np.array_equal(t["palette"].astype(np.float64), c)
    assert ref.truth("tiny-22-6")["initial"] == 5 and ref.truth("tiny-23-8")["initial"] == 7 and ref.truth("tiny-23-8")["M"] == 6


def test_E_is_one_figure_over_all_fixtures():
    E = ref.fixture_E()
    print(f"E = {E:.3e}")
    # the palette is a chain of at most 49 three-by-three solves on numbers of size 1, each a few ulps
    assert 0 < E < 1e-13


def test_the_float64_instance_of_the_statement_makes_the_truths_decisions():
    for name in ("mix-1-24", "tiny-23-8"):
        c, w = ref.fixture(name)
        t, f = ref.truth(name), ref.simplify(c, w, dtype=np.float64)
        assert f["trace"] == t["trace"] and f["stop"] == t["stop"] and np.max(np.abs(f["palette"] - t["palette"])) < 1e-13


@pytest.mark.parametrize("target", [6, 4])
def test_target_size_on_mix_2_44(target):
    c, w = ref.fixture("mix-2-44")
    t = ref.simplify(c, w, target_size=target, dtype=np.longdouble)
    palette, info = extract.simplify_hull_per_op(c, w, target_size=target, return_info=True)
    assert t["trace"] == info["trace"] and palette.shape == (target, 3) and t["M"] == target
    assert info["stop"] == _lib.HULL_STOP[t["stop"]] == "target" and not info["errors"] and not t["errors"]
    assert np.max(np.abs(palette - t["palette"])) < 1e-12
    free = ref.truth("mix-2-44")                     # the collapses are those of the run without a target, cut off (6) or carried on (4)
    n = min(len(free["trace"]), len(t["trace"]))
    assert t["trace"][:n] == free["trace"][:n]


def test_save_palette_and_load_palette_round_trip_and_the_text_format(tmp_path):
    p = np.array([[0.25, 0.5, 1.0], [0.1, 1 / 3, 0.0], [1e-5, 0.7071067811865476, 0.30000000000000004]])
    extract.save_palette(str(tmp_path / "palette.npz"), p)
    with np.load(tmp_path / "palette.npz") as z:
        assert list(z.keys()) == ["palette"] and z["palette"].dtype == np.float64
    assert np.array_equal(extract.load_palette(str(tmp_path / "palette.npz")), p)
    extract.save_palette(str(tmp_path / "extract-palette.txt"), torch.from_numpy(p))
    # write_palette_txt: "r g b" a line, str() of the float64, no newline after the last line
    assert (tmp_path / "extract-palette.txt").read_bytes() == (b"0.25 0.5 1.0\n0.1 0.3333333333333333 0.0\n"
                                                                 b"1e-05 0.7071067811865476 0.30000000000000004")
    assert np.array_equal(extract.load_palette(str(tmp_path / "extract-palette.txt")), p)
    palette, _ = ref.host("mix-1-24")
    extract.save_palette(str(tmp_path / "m-palette.txt"), palette)
    assert np.array_equal(extract.load_palette(str(tmp_path / "m-palette.txt")), palette)           # repr round-trips every float64


def test_simplify_hull_raises_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    c, w = ref.fixture("tiny-22-6")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.simplify_hull(c, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.simplify_hull(torch.tensor(c), torch.tensor(w))


def test_simplify_hull_checks_its_arguments_before_anything_else():
    c, w = ref.fixture("tiny-22-6")
    for bad in (lambda: extract.simplify_hull(c[:3], w[:3]), lambda: extract.simplify_hull(c, w[:5]), lambda: extract.simplify_hull(c, w, error_thres=-1),
                lambda: extract.simplify_hull(c, w, error_thres=float("nan")), lambda: extract.simplify_hull(c, w, target_size=3),
                lambda: extract.simplify_hull(c, w, target_size=17), lambda: extract.simplify_hull(np.zeros((129, 3)), np.ones(129))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("status", [_lib.HULL_COPLANAR, _lib.HULL_FLAT, _lib.HULL_DENSE])
def test_a_hand_over_is_finished_on_the_host_from_the_returned_set(monkeypatch, status):
    """The launch replaced by a stub that answers as the kernel does after three collapses of mix(1, 24): the status, the unclipped vertex
    set the fourth iteration started from, three trace rows.  simplify_hull goes on from there and arrives where the host loop alone does."""
    c, w = ref.fixture("mix-1-24")
    t = ref.truth("mix-1-24")
    palette_host, info_host = ref.host("mix-1-24")
    V, _ = extract._scipy_hull(c)
    for _ in range(3):
        v1, v2, x, _, _ = extract._collapse_per_op(*extract._scipy_hull(V))
        V, _ = extract._scipy_hull(np.vstack((V[[i for i in range(V.shape[0]) if i not in (v1, v2)]], x)))
    calls = []

    def stub(centers, weights, error_thres, target, want_trace=False):
        calls.append((np.asarray(centers).shape, error_thres, target))
        palette = np.zeros((_lib.HULL_MAX_M, 3))
        palette[:min(V.shape[0], 16)] = V[:16]
        return {"info": [status, V.shape[0], 3, t["initial"], 0, 9, 0, 0], "palette": palette, "errors": np.full(8, _lib.HULL_ERROR_NONE),
                "vertices": V.copy(), "trace": np.array(t["trace"][:3], dtype=np.int32)}

    monkeypatch.setattr(extract, "_launch_hull", stub)
    if status == _lib.HULL_FLAT:                    # no hull on the host either
        with pytest.raises(RuntimeError, match="no hull"):
            extract.simplify_hull(c, w)
        return
    palette, info = extract.simplify_hull(c, w, return_info=True)
    assert calls == [((24, 3), 5 / 255, 0)]
    assert info["handed_over"] and info["status"] == status and info["initial"] == t["initial"]
    assert info["trace"] == t["trace"] and info["collapses"] == t["collapses"] and info["stop"] == "error" and info["M"] == t["M"]
    assert np.array_equal(palette, palette_host) and info["errors"] == info_host["errors"]
    assert np.array_equal(extract.simplify_hull(c, w), palette_host)
