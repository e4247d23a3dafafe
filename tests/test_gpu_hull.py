"""pnr_hull_simplify (csrc/hull.hip, include/pnr_hull.h) and palettenerf_amd.extract.simplify_hull / extract_palette on the GPU, against the
longdouble truth of tests/hull_reference.py.

Every integer the kernel reports -- the status, M, the collapses, the initial hull, the stop rule, the largest related-face count, every trace
row, the sizes at which an error was computed -- equals the truth's; the fixtures' margins (tests/test_hull_host.py) keep every such decision
away from rounding.  The palette and the errors are within 4 E of the truth, E being the ONE figure of tests/test_hull_host.py: the largest
distance of the float64 host formulation (scipy / HiGHS) from the truth over all fixtures; the factor covers another, fixed, order of the same
float64 operations (the project's rule, as for the LUT).  mix(4, 40) and mix(8, 40) carry a coplanar facet (see tests/test_hull_host.py): the
kernel refuses them as the truth does and simplify_hull arrives at the host formulation's palette.

Kernel error next to E as measured on an MI355X: see profiles/hull/README.md."""
import ctypes

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, extract, scene
from palettenerf_amd._torch_glue import stream_ptr
from tests import guarded
from tests import hull_reference as ref

pytestmark = pytest.mark.gpu
names = pytest.mark.parametrize("name", ref.NAMES)


def launch(c, w, error_thres=5 / 255, target=0):
    """one launch with every output read back: extract._launch_hull's dict"""
    raw = extract._launch_hull(np.ascontiguousarray(c), np.ascontiguousarray(w), float(error_thres), int(target), want_trace=True)
    raw["errors_by_size"] = {V: raw["errors"][10 - V] for V in range(10, 3, -1) if raw["errors"][10 - V] != _lib.HULL_ERROR_NONE}
    assert raw["errors"][7] == _lib.HULL_ERROR_NONE and raw["info"][6:] == [0, 0]
    return raw


def same_integers(raw, t):
    status, M, collapses, initial, stop, related = raw["info"][:6]
    assert (status, M, collapses, initial, stop, related) == (t["status"], t["M"], t["collapses"], t["initial"], t["stop"], t["related"])
    assert [tuple(int(v) for v in row) for row in raw["trace"]] == t["trace"]
    assert list(raw["errors_by_size"]) == list(t["errors"])


@names
def test_every_fixture_against_the_longdouble_truth(cuda, name):
    t = ref.truth(name)
    E = ref.fixture_E()
    c, w = ref.fixture(name)
    raw = launch(c, w)
    same_integers(raw, t)
    if t["status"] != ref.OK:                       # the coplanar facet of the recipe's clip: refused, the centres returned unclipped
        assert raw["info"][0] == _lib.HULL_COPLANAR and np.array_equal(raw["vertices"], c) and np.array_equal(raw["palette"], c[:16])
        palette, info = extract.simplify_hull(torch.from_numpy(c.copy()).to(cuda), torch.from_numpy(w.copy()).to(cuda), return_info=True)
        want, want_info = ref.host(name)
        assert info["handed_over"] and np.array_equal(palette, want) and info["trace"] == want_info["trace"] and info["initial"] == want_info["initial"]
        return
    M = t["M"]
    got = raw["vertices"]
    assert got.shape == (M, 3) and np.array_equal(got[:16], raw["palette"][:min(M, 16)]) and not raw["palette"][min(M, 16):].any()
    err = float(np.max(np.abs(got - t["palette"])))
    err_e = max((abs(raw["errors_by_size"][V] - e) for V, e in t["errors"].items() if e is not None), default=0.0)
    print(f"{name}: kernel palette error {err:.3e}, error-figure error {float(err_e):.3e}, E {E:.3e}, ratio {err / E:.2f}")
    assert all((e is None) == (raw["errors_by_size"][V] == _lib.HULL_ERROR_FAIL) for V, e in t["errors"].items())
    assert err <= 4 * E, (err, E)
    assert err_e <= 4 * E, (err_e, E)
    assert got.min() >= 0 and got.max() <= 1
    # the Python entrance: the same colours, from device tensors and from host arrays
    p_host, info = extract.simplify_hull(c, w, return_info=True)
    p_dev = extract.simplify_hull(torch.from_numpy(c.copy()).to(cuda), torch.from_numpy(w.copy()).to(cuda))
    assert np.array_equal(p_host, got) and np.array_equal(p_dev, got) and p_host.dtype == np.float64
    assert info["stop"] == _lib.HULL_STOP[t["stop"]] and info["trace"] == t["trace"] and not info["handed_over"] and info["initial"] == t["initial"]


def test_two_launches_give_the_same_bits(cuda):
    for name in ("mix-2-44", "shell-11"):
        c, w = ref.fixture(name)
        a, b = launch(c, w), launch(c, w)
        assert a["info"] == b["info"] and np.array_equal(a["trace"], b["trace"])
        for key in ("palette", "errors", "vertices"):
            assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("target", [6, 4, 9, 16])
def test_target_size(cuda, target):
    c, w = ref.fixture("mix-2-44")
    ref.require_longdouble()
    t = ref.simplify(c, w, target_size=target, dtype=np.longdouble)
    raw = launch(c, w, target=target)
    same_integers(raw, t)
    # 16 is never met (the rule is looked at from 10 vertices down): the run goes on to four, as the reference's does
    assert raw["info"][1] == (target if target <= 10 else 4) and raw["info"][4] == (ref.STOP_TARGET if target <= 10 else ref.STOP_FOUR)
    assert not raw["errors_by_size"]
    assert float(np.max(np.abs(raw["vertices"] - t["palette"]))) <= 4 * ref.fixture_E()
    assert np.array_equal(extract.simplify_hull(c, w, target_size=target), raw["vertices"])


def test_a_target_that_is_stepped_over_runs_on(cuda):
    """tiny(22, 6): five vertices, one collapse, four -- a target of 5 is the initial hull (never looked at: the rule follows a collapse) and is
    stepped over."""
    c, w = ref.fixture("tiny-22-6")
    t = ref.simplify(c, w, target_size=5, dtype=np.longdouble)
    assert t["initial"] == 5 and [row[2] for row in t["trace"]] == [4] and t["stop"] == ref.STOP_FOUR
    raw = launch(c, w, target=5)
    same_integers(raw, t)
    assert float(np.max(np.abs(raw["vertices"] - t["palette"]))) <= 4 * ref.fixture_E()


def test_error_thres_zero_stops_at_the_first_check_and_a_huge_one_runs_to_four(cuda):
    c, w = ref.fixture("mix-2-44")
    E = ref.fixture_E()
    for thres, stop, M in ((0.0, ref.STOP_ERROR, 11), (1e9, ref.STOP_FOUR, 4)):
        t = ref.simplify(c, w, error_thres=thres, dtype=np.longdouble)
        assert (t["stop"], t["M"]) == (stop, M)
        raw = launch(c, w, error_thres=thres)
        same_integers(raw, t)
        assert float(np.max(np.abs(raw["vertices"] - t["palette"]))) <= 4 * E
        assert max(abs(raw["errors_by_size"][V] - e) for V, e in t["errors"].items()) <= 4 * E
    assert list(raw["errors_by_size"]) == [10, 9, 8, 7, 6, 5, 4]


@pytest.mark.parametrize("name", ["tiny-20-4", "tiny-21-5"])
def test_four_and_five_centres_return_the_input_hull(cuda, name):
    c, w = ref.fixture(name)
    raw = launch(c, w)
    assert raw["info"][:5] == [_lib.HULL_OK, c.shape[0], 0, c.shape[0], ref.STOP_UNCHANGED] and raw["trace"].shape == (0, 4)
    assert np.array_equal(raw["vertices"], c)       # inside [0,1]: the clip changes nothing


def test_the_largest_launch_terminates_and_matches_the_host_formulations_trace(cuda):
    """128 shell points: 88 hull vertices, 81 collapses.  The host formulation needs about 40 s for it, so its run is a recorded result
    (tests/golden/hull_shell128_host.npz, written by hull_reference.save_shell128)."""
    c, w = ref.shell128()
    want = ref.load_shell128()
    raw = launch(c, w)
    status, M, collapses, initial, stop, related = raw["info"][:6]
    assert status == _lib.HULL_OK and collapses <= 128 - 4 and collapses == len(want["trace"]) == 81
    assert [tuple(int(v) for v in row) for row in raw["trace"]] == want["trace"]
    assert (M, initial, stop, related) == (want["palette"].shape[0], want["initial"], want["stop"], want["related"])
    assert list(raw["errors_by_size"]) == list(want["errors"])
    d = float(np.max(np.abs(raw["vertices"] - want["palette"])))
    print(f"shell128: kernel - host formulation {d:.3e}")
    # no truth at this size: two float64 evaluations of 81 chained three-by-three solves on numbers of size 1
    assert d < 1e-12 and max(abs(raw["errors_by_size"][V] - e) for V, e in want["errors"].items()) < 1e-12


def test_interior_centres_are_dropped(cuda):
    c, w, order = ref.interior_case()
    t = ref.simplify(c, w, dtype=np.longdouble)
    assert t["initial"] == ref.truth("tiny-23-8")["initial"] == 7
    raw = launch(c, w)
    same_integers(raw, t)
    assert float(np.max(np.abs(raw["vertices"] - t["palette"]))) <= 4 * ref.fixture_E()
    # the collapses are those of the eight points alone, in the shuffled numbering's order of the same hull
    assert [row[2:] for row in t["trace"]] == [row[2:] for row in ref.truth("tiny-23-8")["trace"]]


def test_a_coplanar_facet_is_handed_over_and_finished_on_the_host(cuda):
    c, w = ref.coplanar_case()
    raw = launch(c, w)
    assert raw["info"][:5] == [_lib.HULL_COPLANAR, 40, 0, 0, ref.STOP_NONE]
    assert np.array_equal(raw["vertices"], c) and np.array_equal(raw["palette"], c[:16]) and raw["trace"].shape == (0, 4)
    palette, info = extract.simplify_hull(c, w, return_info=True)
    want, want_info = extract.simplify_hull_per_op(c, w, return_info=True)
    assert info["handed_over"] and "fourth point" in info["handed_over"] and info["status"] == _lib.HULL_COPLANAR
    assert np.array_equal(palette, want) and info["trace"] == want_info["trace"] and info["stop"] == want_info["stop"]
    assert 4 <= palette.shape[0] <= 10 and palette.min() >= 0 and palette.max() <= 1 and not info["errors"][palette.shape[0]] > 5 / 255


def test_a_flat_set_is_refused(cuda):
    c, w = ref.flat_case()
    raw = launch(c, w)
    assert raw["info"][:5] == [_lib.HULL_FLAT, 12, 0, 0, ref.STOP_NONE] and np.array_equal(raw["vertices"], c)
    with pytest.raises(RuntimeError, match="no hull"):
        extract.simplify_hull(c, w)


def test_an_apex_above_the_related_face_cap_is_handed_over(cuda):
    c, w = ref.dense_case()
    t = ref.simplify(c, w, dtype=np.float64, dense_cap=_lib.HULL_MAX_RELATED)
    assert t["status"] == ref.DENSE and t["related"] == 72 > _lib.HULL_MAX_RELATED
    raw = launch(c, w)
    assert raw["info"][:6] == [_lib.HULL_DENSE, 72, 0, 72, ref.STOP_NONE, 72]
    assert np.array_equal(raw["vertices"], c)       # every centre is a vertex: the set the first iteration started from
    # (finishing this one on the host is some sixty collapses of HiGHS calls: the finish from a DENSE status is tests/test_hull_host.py's)


# ---------------------------------------------------------------- guard bands
def guarded_launch(cuda, c, w, align64, align32):
    c_buf, c_view = guarded.inp(torch.from_numpy(c.copy()).to(cuda), align64)
    w_buf, w_view = guarded.inp(torch.from_numpy(w.copy()).to(cuda), align64)
    K = c.shape[0]
    outs = {"palette": guarded.out((_lib.HULL_MAX_M, 3), torch.float64, cuda, align64), "info": guarded.out((8,), torch.int32, cuda, align32),
            "errors": guarded.out((8,), torch.float64, cuda, align64), "trace": guarded.out((K, 4), torch.int32, cuda, align32),
            "vertices": guarded.out((K, 3), torch.float64, cuda, align64)}
    a = _lib.HullSimplifyArgs()
    a.centers, a.center_weights, a.K, a.error_thres, a.target_size = c_view.data_ptr(), w_view.data_ptr(), K, 5 / 255, 0
    for name, (_, view) in outs.items():
        assert view.data_ptr() % 256 == (align32 if view.dtype == torch.int32 else align64) % 256
        setattr(a, name, view.data_ptr())
    rc = _lib.load().pnr_hull_simplify(ctypes.byref(a), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    for name, (buf, view) in (*outs.items(), ("centers", (c_buf, c_view)), ("center_weights", (w_buf, w_view))):
        assert guarded.untouched(buf, view), f"{name}: {guarded.last_report}"
    return {name: view.cpu().numpy() for name, (_, view) in outs.items()}


@pytest.mark.parametrize("align64,align32", [(256, 256), (8, 4)], ids=["256-byte", "weakest"])
@pytest.mark.parametrize("name", ["mix-1-24", "shell-11", "mix-4-40"])
def test_no_byte_outside_the_arrays_is_written_or_used(cuda, name, align64, align32):
    """Sentinel bytes around palette, info, errors, trace and vertices, NaNs around centers and center_weights, at a 256-byte alignment and at
    the weakest the header documents (8 bytes for float64, 4 for int32); the outputs equal the plain call's bit for bit.  mix-4-40 is the
    hand-over, whose vertex set fills all K rows."""
    c, w = ref.fixture(name)
    plain = launch(c, w)
    got = guarded_launch(cuda, c, w, align64, align32)
    M, collapses = plain["info"][1], plain["info"][2]
    assert got["info"].tolist() == plain["info"]
    assert got["palette"][:min(M, 16)].tobytes() == plain["palette"][:min(M, 16)].tobytes()
    assert got["errors"].tobytes() == plain["errors"].tobytes()
    assert got["vertices"][:M].tobytes() == plain["vertices"].tobytes() and np.array_equal(got["trace"][:collapses], plain["trace"])
    # rows the call does not return keep the caller's bytes
    sentinel = np.frombuffer(bytes([guarded.SENTINEL]) * 8, dtype=np.float64)[0]
    assert (got["vertices"][M:].view(np.uint64) == sentinel.view(np.uint64)).all()
    assert (got["trace"][collapses:].view(np.uint8) == guarded.SENTINEL).all()


def test_the_optional_outputs_may_be_absent(cuda):
    c, w = ref.fixture("mix-1-24")
    plain = launch(c, w)
    cd, wd = torch.from_numpy(c.copy()).to(cuda), torch.from_numpy(w.copy()).to(cuda)
    palette = torch.zeros(_lib.HULL_MAX_M, 3, dtype=torch.float64, device=cuda)
    info = torch.zeros(8, dtype=torch.int32, device=cuda)
    a = _lib.HullSimplifyArgs()
    a.centers, a.center_weights, a.K, a.error_thres, a.target_size = cd.data_ptr(), wd.data_ptr(), c.shape[0], 5 / 255, 0
    a.palette, a.info = palette.data_ptr(), info.data_ptr()
    assert _lib.load().pnr_hull_simplify(ctypes.byref(a), stream_ptr()) == 0
    assert info.cpu().tolist() == plain["info"] and np.array_equal(palette.cpu().numpy(), plain["palette"])


# ---------------------------------------------------------------- end to end
def test_extract_palette_is_the_three_steps_in_one_call(cuda):
    from tests.test_gpu_extract import KW, fence_free_images
    from tests.test_gpu_jitter import make_model
    from tests.test_gpu_lut import small_model
    H = W = 16
    m = make_model("nerf", cuda, 0, 100.0)
    intr = scene.intrinsics_from_fov(H, W)
    poses = np.stack([scene.lookat_pose(azimuth_deg=30.0 + 40.0 * i) for i in range(3)])
    images = torch.from_numpy(fence_free_images(3, H, W, "fp32", 11))
    res = extract.extract_centers(m, poses, intr, H, W, images, tau=0.02, **KW)
    K = res["info"]["K"]
    assert K >= 4
    want = extract.simplify_hull(res["centers"], res["center_weights"], target_size=6)
    print(f"end to end: K {K}, palette {want.shape[0]} colours")
    assert 4 <= want.shape[0] <= 16
    pm = small_model(cuda, want.shape[0])
    palette, lut, res2 = extract.extract_palette(m, poses, intr, H, W, images, palette_model=pm, palette_size=6, normalize_input=True, tau=0.02, **KW)
    assert np.array_equal(res2["centers"], res["centers"]) and np.array_equal(res2["center_weights"], res["center_weights"])
    assert np.array_equal(palette, want)
    assert torch.equal(lut, extract.weight_lut(want, normalize_input=True, device=cuda)) and torch.equal(pm.hist_weights.data, lut)
    assert torch.equal(pm.basis_color.detach().cpu(), torch.from_numpy(want).float())
    # without a palette model the LUT is built on the NeRF model's device; the error rule decides the size
    palette2, lut2, _ = extract.extract_palette(m, poses, intr, H, W, images, tau=0.02, **KW)
    assert np.array_equal(palette2, extract.simplify_hull(res["centers"], res["center_weights"]))
    assert torch.equal(lut2, extract.weight_lut(palette2, device=cuda)) and lut2.shape[1] == palette2.shape[0]
