"""The palette weight LUT on the host (no GPU): the closed statement of tests/lut_reference.py against a chain that follows the reference's
lines with scipy (ConvexHull, Delaunay.find_simplex(tol=1e-8), per-tetrahedron Delaunay.transform), both against the longdouble truth --
the larger of the two errors is a fixture's E, the yardstick tests/test_gpu_lut.py holds the kernel to --, extract's host formulation, the
palette and LUT files, and the C ABI of pnr_lut_weights: declared, bound, mirrored, and refusing before a launch.

E as measured (float64 formulation | scipy chain, max over the 32 768 bins and the columns): see profiles/lut/README.md."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from palettenerf_amd import _lib, extract
from tests import lut_reference as ref

INVALID, UNSUPPORTED = -1, -2
P = 64      # a non-null, 16-byte aligned address that is never read
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnr.h")
fixtures = pytest.mark.parametrize("name,normalize", ref.FIXTURES, ids=ref.FIXTURE_IDS)


def scipy_chain(points, palette):
    """Additive_mixing_layers_extraction.py:397-547 in its line order: the order by L1 distance to black, ConvexHull and Delaunay of the
    ordered palette, find_simplex(tol=1e-8) for the outside points, each replaced by the nearest of the closest points on the hull's
    triangles; then for every hull simplex without vertex 0, in qhull's order, the Delaunay of (V[0], Vi, Vj, Vk), the still unassigned
    points it contains (tol=1e-8), and their barycentrics from its transform; the columns back to the caller's order."""
    from scipy.spatial import ConvexHull, Delaunay
    palette = np.asarray(palette, dtype=np.float64)
    order = np.argsort(np.abs(palette).sum(axis=-1), kind="stable")
    V = palette[order]
    x = np.array(points, dtype=np.float64).reshape(-1, 3)
    hull = ConvexHull(V)
    outside = Delaunay(V).find_simplex(x, tol=1e-8) < 0
    if outside.any():
        xo = x[outside]
        cand = np.stack([ref.closest_on_triangle(xo, *hull.points[s]) for s in hull.simplices], axis=1)
        dist = np.sqrt(((xo[:, None, :] - cand) ** 2).sum(axis=-1))
        x[outside] = cand[np.arange(xo.shape[0]), np.argmin(dist, axis=1)]
    assert (Delaunay(V).find_simplex(x, tol=1e-8) >= 0).all()
    W = np.zeros((x.shape[0], V.shape[0]))
    left = np.arange(x.shape[0])
    for face in hull.simplices:
        if not (face != 0).all() or left.size == 0:
            continue
        corners = np.array([0] + sorted(int(v) for v in face))
        tet = Delaunay(V[corners])
        inside = tet.find_simplex(x[left], tol=1e-8) >= 0
        chosen = left[inside]
        left = left[~inside]
        b = np.einsum("jk,nk->nj", tet.transform[0, :3], x[chosen] - tet.transform[0, 3])
        W[chosen[:, None], corners[tet.simplices[0]][None, :]] = np.c_[b, 1 - b.sum(axis=1)]
    assert left.size == 0, f"{left.size} points in no star tetrahedron"
    out = np.ones_like(W)
    out[:, order] = W
    return out, outside


@functools.lru_cache(maxsize=None)
def fixture_errors(name, normalize):
    """(error of the float64 formulation, error of the scipy chain) against the longdouble truth: max over bins and columns."""
    truth, info = ref.truth(name, normalize)
    w64, info64 = ref.float64_formulation(name, normalize)
    chain, outside = scipy_chain(ref.bin_points(normalize), ref.PALETTES[name])
    assert np.array_equal(info["outside"], info64["outside"]) and np.array_equal(info["outside"], outside)
    return float(np.max(np.abs(w64 - truth))), float(np.max(np.abs(chain - truth)))


def fixture_error(name, normalize):
    """E of a fixture: the larger of the two float64 formulations' errors."""
    return max(fixture_errors(name, normalize))


@fixtures
def test_the_two_float64_formulations_agree_with_the_longdouble_truth(name, normalize):
    ref.require_longdouble()
    truth, info = ref.truth(name, normalize)
    e64, echain = fixture_errors(name, normalize)
    n_out = int(info["outside"].sum())
    print(f"{name} normalize={normalize}: outside {n_out} of 32768, margin {info['margin']:.3e}, E float64 {e64:.3e}, E scipy chain {echain:.3e}")
    assert info["margin"] >= ref.MIN_MARGIN
    assert 13000 <= n_out <= 32768
    # two float64 evaluations of a continuous function with weights of size 1 and hull edges of size 0.5: a few hundred ulps at the most
    assert 0 < max(e64, echain) < 1e-12
    # extract's own host formulation (the kernel's operation order) is a third float64 evaluation of the same function
    W = extract.palette_weights_per_op(ref.bin_points(False), ref.PALETTES[name], normalize_input=normalize)
    assert np.max(np.abs(W - truth)) < 1e-12


@fixtures
def test_rows_sum_to_one_are_not_negative_and_reproduce_the_point(name, normalize):
    palette = ref.PALETTES[name]
    for W, info in (ref.float64_formulation(name, normalize), extract.palette_weights_per_op(ref.bin_points(normalize), palette, return_info=True)):
        assert np.max(np.abs(W.sum(axis=1) - 1)) < 1e-12 and W.min() >= -1e-12
        assert (np.count_nonzero(W, axis=1) <= 4).all()
        x = ref.bin_points(normalize)
        mixed = W @ palette
        inside = ~info["outside"]
        assert not inside.any() or np.max(np.abs(mixed[inside] - x[inside])) < 1e-12     # an inside point is reproduced (P4 normalised has none)
        assert np.max(np.abs(mixed - info["projected"])) < 1e-12                  # an outside one gives its projection
        moved = np.linalg.norm(info["projected"] - x, axis=1)
        assert (moved[info["outside"]] > 1e-8).all() and (moved[inside] == 0).all()


def test_an_interior_palette_row_gets_a_zero_column_and_a_permuted_palette_permuted_columns():
    x = ref.bin_points(True)
    inner = ref.P8.mean(axis=0)
    P9 = np.concatenate([ref.P8[:3], inner[None], ref.P8[3:]])
    for fn in (lambda p: ref.weights(x, p)[0], lambda p: extract.palette_weights_per_op(x, p)):
        W8, W9 = fn(ref.P8), fn(P9)
        assert (W9[:, 3] == 0).all() and np.array_equal(np.delete(W9, 3, axis=1), W8)
        perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
        assert np.array_equal(fn(ref.P8[perm]), W8[:, perm])
    assert 3 not in ref.weights(x, P9)[1]["hull_vertices"]


def test_flat_and_coplanar_palettes_are_refused():
    flat = np.array([[.1, .1, .2], [.9, .1, .2], [.1, .9, .2], [.9, .9, .2], [.5, .4, .2]])
    cube = np.array([[r, g, b] for r in (.1, .9) for g in (.1, .9) for b in (.1, .9)], dtype=np.float64)
    with pytest.raises(ValueError, match="flat"):
        ref.hull_faces(flat[ref.hull_order(flat)])
    with pytest.raises(ValueError, match="coplanar"):
        ref.hull_faces(cube[ref.hull_order(cube)])
    with pytest.raises(RuntimeError, match="no hull"):
        extract.palette_hull(flat)
    with pytest.raises(RuntimeError, match="fourth colour"):
        extract.palette_hull(cube)
    for bad in (ref.P6[:3], np.zeros((17, 3))):
        with pytest.raises(ValueError, match="4..16"):
            extract.palette_hull(bad)


def test_weight_lut_per_op_has_the_reference_layout():
    hw = extract.weight_lut_per_op(ref.P6, normalize_input=True)
    assert hw.shape == (32, 32, 32, 6) and hw.dtype == np.float64
    W = extract.palette_weights_per_op(ref.bin_points(True), ref.P6)
    code = (7 << 10) | (19 << 5) | 30
    assert np.array_equal(hw[7, 19, 30], W[code]) and np.array_equal(hw.reshape(-1, 6), W)
    # normalize_input on the bin centres is the normalisation of tests/lut_reference.py, bit for bit
    assert np.array_equal(hw.reshape(-1, 6), extract.palette_weights_per_op(extract.bin_centers_of(5), ref.P6, normalize_input=True))


def test_load_palette_reads_both_files_of_the_reference(tmp_path):
    np.savez(tmp_path / "palette.npz", palette=ref.P6)
    assert np.array_equal(extract.load_palette(str(tmp_path / "palette.npz")), ref.P6)
    # write_palette_txt's format: "r g b" a line, str() of the float64, no newline after the last
    text = "\n".join(f"{c[0]} {c[1]} {c[2]}" for c in ref.P8)
    (tmp_path / "extract-palette.txt").write_text(text)
    got = extract.load_palette(str(tmp_path / "extract-palette.txt"))
    assert got.dtype == np.float64 and np.array_equal(got, ref.P8)
    (tmp_path / "bad-palette.txt").write_text("0.1 0.2\n0.3 0.4\n")
    with pytest.raises(ValueError):
        extract.load_palette(str(tmp_path / "bad-palette.txt"))


def test_save_lut_and_load_lut_round_trip_and_read_the_reference_file(tmp_path):
    import torch
    hw = extract.weight_lut_per_op(ref.P4)
    lut = torch.as_tensor(hw).float().permute(3, 0, 1, 2).unsqueeze(0).contiguous()      # as the model keeps it
    extract.save_lut(str(tmp_path / "ours.npz"), lut)
    with np.load(tmp_path / "ours.npz") as z:
        assert list(z.keys()) == ["hist_weights"] and z["hist_weights"].shape == (32, 32, 32, 4) and z["hist_weights"].dtype == np.float64
    back = extract.load_lut(str(tmp_path / "ours.npz"))
    assert np.array_equal(back, hw.astype(np.float32).astype(np.float64))
    assert torch.equal(extract.load_lut(str(tmp_path / "ours.npz"), device="cpu"), lut)
    np.savez(tmp_path / "hist_weights.npz", hist_weights=hw)                                # the reference's own file: palette/utils.py:254
    assert np.array_equal(extract.load_lut(str(tmp_path / "hist_weights.npz")), hw)
    assert torch.equal(extract.load_lut(str(tmp_path / "hist_weights.npz"), device="cpu"), lut)
    extract.save_lut(str(tmp_path / "host.npz"), hw)                                       # a host table is saved as it is
    assert np.array_equal(extract.load_lut(str(tmp_path / "host.npz")), hw)
    assert np.array_equal(extract.lut_to_hist_weights(lut), back)


# ---------------------------------------------------------------- the C ABI
def lut_args(**over):
    a = _lib.LutWeightsArgs()
    a.palette = a.points = a.weights64 = a.lut32 = a.info = P
    a.M, a.N, a.points_format, a.point_stride = 6, 100, _lib.LUT_POINTS_FP32, 3
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_entry_is_declared_bound_and_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    header = open(HEADER).read()
    assert re.search(r"\bint pnr_lut_weights\(const pnr_lut_weights_args\* args, pnr_stream_t stream\);", header)
    assert _lib.SIGNATURES["pnr_lut_weights"] == [ctypes.c_void_p, ctypes.c_void_p] and hasattr(lib, "pnr_lut_weights")
    for macro, value in (("PNR_LUT_MIN_M", _lib.LUT_MIN_M), ("PNR_LUT_MAX_M", _lib.LUT_MAX_M), ("PNR_LUT_MAX_FACES", _lib.LUT_MAX_FACES),
                         ("PNR_LUT_POINTS_BINS", _lib.LUT_POINTS_BINS), ("PNR_LUT_POINTS_FP32", _lib.LUT_POINTS_FP32),
                         ("PNR_LUT_POINTS_FP64", _lib.LUT_POINTS_FP64), ("PNR_LUT_OK", _lib.LUT_OK), ("PNR_LUT_FLAT", _lib.LUT_FLAT),
                         ("PNR_LUT_COPLANAR", _lib.LUT_COPLANAR)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert (_lib.LUT_MIN_M, _lib.LUT_MAX_M, _lib.LUT_MAX_FACES) == (4, 16, 2 * 16 - 4)


def test_the_struct_mirror_has_the_layout_gcc_gives_the_header_struct(tmp_path):
    mirror = _lib.LutWeightsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(pnr_lut_weights_args));']
    lines += [f'  printf("{f[0]} %zu\\n", offsetof(pnr_lut_weights_args, {f[0]}));' for f in mirror._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(mirror)
    for f in mirror._fields_:
        assert int(got[f[0]]) == getattr(mirror, f[0]).offset, f[0]
    body = re.search(r"typedef struct pnr_lut_weights_args \{(.*?)\} pnr_lut_weights_args;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert sum(len(d.split(",")) for d in body.split(";") if d.strip()) == len(mirror._fields_)


def test_the_entry_refuses_before_a_launch():
    fn = _lib.load().pnr_lut_weights
    assert fn(None, None) == INVALID
    for name in ("palette", "info", "points"):
        assert fn(ctypes.byref(lut_args(**{name: None})), None) == INVALID, name
    assert fn(ctypes.byref(lut_args(weights64=None, lut32=None)), None) == INVALID                  # neither output
    for M in (0, 1, 3, 17, 1 << 20):
        assert fn(ctypes.byref(lut_args(M=M)), None) == INVALID, M
    for fmt in (-1, 3, 9):
        assert fn(ctypes.byref(lut_args(points_format=fmt)), None) == UNSUPPORTED, fmt
    assert fn(ctypes.byref(lut_args(M=3, points_format=9)), None) == INVALID                        # M is looked at first
    assert fn(ctypes.byref(lut_args(point_stride=2)), None) == INVALID
    assert fn(ctypes.byref(lut_args(points=P + 2)), None) == INVALID
    assert fn(ctypes.byref(lut_args(points=P + 4, points_format=_lib.LUT_POINTS_FP64)), None) == INVALID
    assert fn(ctypes.byref(lut_args(palette=P + 4)), None) == INVALID
    assert fn(ctypes.byref(lut_args(weights64=P + 4)), None) == INVALID
    assert fn(ctypes.byref(lut_args(lut32=P + 2)), None) == INVALID
    # the generated points are the 32 768 bins, and take no array
    assert fn(ctypes.byref(lut_args(points_format=_lib.LUT_POINTS_BINS, N=32768)), None) == INVALID
    assert fn(ctypes.byref(lut_args(points_format=_lib.LUT_POINTS_BINS, points=None, N=32767)), None) == INVALID


def test_launch_geometry_answers_for_the_entry():
    assert _lib.launch_geometry("pnr_lut_weights", 1) == (1, 128)
    assert _lib.launch_geometry("pnr_lut_weights", 129) == (2, 128)
    assert _lib.launch_geometry("pnr_lut_weights", 32768) == (256, 128)
    cap, tile = _lib.launch_geometry("pnr_lut_weights", 1 << 31)
    assert tile == 128 and _lib.launch_geometry("pnr_lut_weights", cap * tile) == (cap, tile) and _lib.launch_geometry("pnr_lut_weights", cap * tile + 1) == (cap, tile)
    wg, rpt = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert _lib.load().pnr_launch_geometry(b"pnr_lut_weights", 1 << 32, ctypes.byref(wg), ctypes.byref(rpt)) == INVALID and (wg.value, rpt.value) == (7, 7)
