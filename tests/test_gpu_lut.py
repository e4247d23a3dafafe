"""pnr_lut_weights (csrc/lut.hip) and palettenerf_amd.extract's weight LUT on the GPU, against the longdouble truth of tests/lut_reference.py.

The bound of the LUT case is 4 x E of the fixture, E being the larger error of the two float64 host formulations against the same truth
(tests/test_lut_host.py: fixture_error): the factor covers another, fixed, order of the same float64 operations.  Everything else here is
exact: the fp32 table is the float64 result rounded once, a launch repeats its bits, a row does not depend on its batch, its source format
or its stride, a palette row inside the hull gets zeros and changes nothing else, a permuted palette permutes the columns.

Kernel error / E as measured on an MI355X (max over the 32 768 bins and the columns): see profiles/lut/README.md."""
import ctypes

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, extract, palette_utils, trainset
from palettenerf_amd._torch_glue import stream_ptr
from tests import lut_reference as ref
from tests.test_lut_host import fixture_error

pytestmark = pytest.mark.gpu
fixtures = pytest.mark.parametrize("name,normalize", ref.FIXTURES, ids=ref.FIXTURE_IDS)
SENTINEL = -7.25


def as_reference_layout(w64):
    """initialize_palette's own expression on the [32,32,32,M] float64 table"""
    return torch.as_tensor(w64.reshape(32, 32, 32, -1)).float().permute(3, 0, 1, 2).unsqueeze(0)


@fixtures
def test_the_lut_is_within_four_e_of_the_longdouble_truth(cuda, name, normalize):
    truth, info = ref.truth(name, normalize)
    E = fixture_error(name, normalize)
    lut, w64 = extract.weight_lut(ref.PALETTES[name], normalize_input=normalize, device=cuda, return_weights64=True)
    assert lut.shape == (1, truth.shape[1], 32, 32, 32) and lut.dtype == torch.float32 and lut.device.type == "cuda"
    assert w64.shape == truth.shape and w64.dtype == torch.float64
    w = w64.cpu().numpy()
    err = float(np.max(np.abs(w - truth)))
    print(f"{name} normalize={normalize}: kernel error {err:.3e}, E {E:.3e}, ratio {err / E:.2f}")
    assert err <= 4 * E, (err, E)
    assert np.max(np.abs(w.sum(axis=1) - 1)) < 1e-12 and w.min() >= -1e-12 and (np.count_nonzero(w, axis=1) <= 4).all()
    # the fp32 table: the float64 results rounded once, in the model's layout, bit for bit; and the same bits from a second launch
    assert torch.equal(lut.cpu(), as_reference_layout(w))
    again, w64_again = extract.weight_lut(ref.PALETTES[name], normalize_input=normalize, device=cuda, return_weights64=True)
    assert torch.equal(again, lut) and torch.equal(w64_again, w64)
    # the table alone (no float64 output asked for) holds the same bits
    assert torch.equal(extract.weight_lut(ref.PALETTES[name], normalize_input=normalize, device=cuda), lut)


def second_trip_batch():
    wg, tile = _lib.launch_geometry("pnr_lut_weights", 1 << 31)
    n = wg * tile + 1
    assert _lib.launch_geometry("pnr_lut_weights", n) == (wg, tile) and n > wg * tile           # one row on a second trip
    return n, tile


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalised"])
def test_an_array_of_points_gives_the_rows_of_the_lut_whatever_its_size_format_and_stride(cuda, normalize):
    big, tile = second_trip_batch()
    x = torch.from_numpy(ref.bin_points(False)).to(cuda)                   # float64, and exact in float32
    reps = -(-big // x.shape[0])
    pts = x.repeat(reps, 1)[:big].contiguous()
    _, w_bins = extract.weight_lut(ref.P6, normalize_input=normalize, device=cuda, return_weights64=True)
    w_big = extract.palette_weights(pts, ref.P6, normalize_input=normalize)
    assert w_big.shape == (big, 6) and w_big.dtype == torch.float64
    # the generated bins and the uploaded ones are the same points: the same bits, on every trip of the tile loop
    assert torch.equal(w_big, w_bins.repeat(reps, 1)[:big])
    for n in (1, 63, 64, 65, tile - 1, tile, tile + 1, 257):
        sub = pts[5000:5000 + n]
        w = extract.palette_weights(sub, ref.P6, normalize_input=normalize)
        assert w.shape == (n, 6) and torch.equal(w, w_big[5000:5000 + n]), n
        # fp32 points (the bin centres are exact in fp32)
        assert torch.equal(extract.palette_weights(sub.float(), ref.P6, normalize_input=normalize), w), n
        # columns 1..3 of an [n,5] tensor, read in place
        wide = torch.full((n, 5), 9.0, dtype=torch.float64, device=cuda)
        wide[:, 1:4] = sub
        view = wide[:, 1:4]
        assert view.stride() == (5, 1) and view.data_ptr() == wide.data_ptr() + 8 and (n == 1 or not view.is_contiguous())
        assert torch.equal(extract.palette_weights(view, ref.P6, normalize_input=normalize), w), n
        assert torch.equal(extract.palette_weights(wide.float()[:, 1:4], ref.P6, normalize_input=normalize), w), n
        # fp32 output: [n,M], the float64 rounded once
        assert torch.equal(extract.palette_weights(sub, ref.P6, out_dtype=torch.float32, normalize_input=normalize), w.float()), n
    # the last rows of the big launch -- the second trip -- against a fresh launch on the same rows
    tail = pts[big - 3:].clone()
    assert torch.equal(extract.palette_weights(tail, ref.P6, normalize_input=normalize), w_big[big - 3:])
    # leading dimensions are kept
    assert extract.palette_weights(pts[:24].reshape(2, 3, 4, 3), ref.P6).shape == (2, 3, 4, 6)


def test_points_off_the_bin_centres_against_the_truth(cuda):
    """random colours, some far outside [0,1]: fp64 and fp32 arrays against the longdouble statement on the same numbers"""
    ref.require_longdouble()
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.random((700, 3)), rng.random((163, 3)) * 3 - 1])
    for dtype in (np.float64, np.float32):
        pts = x.astype(dtype)
        truth, info = ref.weights(pts.astype(np.float64), ref.P8, dtype=np.longdouble, cramer=True)
        w64, _ = ref.weights(pts.astype(np.float64), ref.P8)
        if info["margin"] < ref.MIN_MARGIN:
            pytest.fail(f"bad fixture: a point within {info['margin']} of the inside/outside rule")
        E = float(np.max(np.abs(w64 - truth)))
        w = extract.palette_weights(torch.from_numpy(pts).to(cuda), ref.P8).cpu().numpy()
        err = float(np.max(np.abs(w - truth)))
        print(f"random {np.dtype(dtype).name}: kernel error {err:.3e}, float64 formulation {E:.3e}")
        # points up to 2 away from the hull: the projection's operands are up to 4x the bins', so is an ulp of them
        assert err <= 4 * max(E, 4 * 2.0 ** -52), (err, E)


def test_an_interior_palette_row_gets_zeros_and_a_permuted_palette_permuted_columns(cuda):
    lut8, w8 = extract.weight_lut(ref.P8, normalize_input=True, device=cuda, return_weights64=True)
    inner = ref.P8.mean(axis=0)
    P9 = np.concatenate([ref.P8[:3], inner[None], ref.P8[3:]])
    lut9, w9 = extract.weight_lut(P9, normalize_input=True, device=cuda, return_weights64=True)
    keep = [0, 1, 2, 4, 5, 6, 7, 8]
    assert bool((w9[:, 3] == 0).all()) and bool((lut9[0, 3] == 0).all())
    assert torch.equal(w9[:, keep], w8) and torch.equal(lut9[:, keep], lut8)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    lutp, wp = extract.weight_lut(ref.P8[perm], normalize_input=True, device=cuda, return_weights64=True)
    assert torch.equal(wp, w8[:, perm]) and torch.equal(lutp, lut8[:, perm])
    # sixteen colours, the compiled cap: P8 and eight colours inside its hull
    rng = np.random.default_rng(3)
    mix = rng.dirichlet(np.ones(8), size=8) * 0.9 + 0.1 / 8
    P16 = np.concatenate([ref.P8, mix @ ref.P8])
    lut16 = extract.weight_lut(P16, normalize_input=True, device=cuda)
    assert torch.equal(lut16[:, :8], lut8) and bool((lut16[:, 8:] == 0).all())


def raw_launch(cuda, palette, n_out):
    """pnr_lut_weights on the bins with both outputs pre-filled: (return code, info, weights64, lut32)"""
    pal = torch.from_numpy(np.ascontiguousarray(palette, dtype=np.float64)).to(cuda)
    M = pal.shape[0]
    w64 = torch.full((n_out, M), SENTINEL, dtype=torch.float64, device=cuda)
    w32 = torch.full((M, n_out), SENTINEL, dtype=torch.float32, device=cuda)
    info = torch.full((4,), -1, dtype=torch.int32, device=cuda)
    a = _lib.LutWeightsArgs()
    a.palette, a.M, a.points, a.points_format, a.point_stride, a.N = pal.data_ptr(), M, None, _lib.LUT_POINTS_BINS, 3, n_out
    a.weights64, a.lut32, a.info = w64.data_ptr(), w32.data_ptr(), info.data_ptr()
    rc = _lib.load().pnr_lut_weights(ctypes.byref(a), stream_ptr())
    torch.cuda.synchronize()
    return rc, info.cpu().tolist(), w64, w32


def test_a_flat_palette_and_a_cube_are_refused_and_nothing_is_written(cuda):
    flat = np.array([[.1, .1, .2], [.9, .1, .2], [.1, .9, .2], [.9, .9, .2], [.5, .4, .2]])
    cube = np.array([[r, g, b] for r in (.1, .9) for g in (.1, .9) for b in (.1, .9)], dtype=np.float64)
    for palette, status, text in ((flat, _lib.LUT_FLAT, "no hull"), (cube, _lib.LUT_COPLANAR, "fourth colour")):
        rc, info, w64, w32 = raw_launch(cuda, palette, 32768)
        assert rc == 0 and info[0] == status and info[1] == 0
        assert bool((w64 == SENTINEL).all()) and bool((w32 == SENTINEL).all())
        with pytest.raises(RuntimeError, match=text):
            extract.weight_lut(palette, device=cuda)
        with pytest.raises(RuntimeError, match=text):
            extract.palette_weights(torch.rand(10, 3, device=cuda), palette)
    rc, info, w64, w32 = raw_launch(cuda, ref.P6, 32768)                 # the same call on a palette with a hull: 8 faces, 4 of them without V[0]
    assert rc == 0 and info == [_lib.LUT_OK, 8, info[2], 0] and 1 <= info[2] < 8
    assert not bool((w64 == SENTINEL).any()) and not bool((w32 == SENTINEL).any())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.palette_weights(torch.rand(10, 3), ref.P6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract.weight_lut(ref.P6, device="cpu")


def small_model(cuda, num_basis):
    from palettenerf_amd import network, renderer, scene
    torch.manual_seed(0)
    m = network.PaletteNetwork(renderer.default_opt(test=False, num_basis=num_basis), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    return m.to(cuda)


def test_initialize_from_extraction_feeds_the_model_the_guide_and_the_training_batch(cuda):
    m = small_model(cuda, 6)
    lut = extract.initialize_from_extraction(m, ref.P6, normalize_input=True)
    hw = m.hist_weights
    assert tuple(hw.shape) == (1, 6, 32, 32, 32) and hw.dtype == torch.float32 and hw.device.type == "cuda" and not hw.requires_grad
    assert hw.is_contiguous() and torch.equal(hw.data, lut)
    assert torch.equal(m.basis_color.detach().cpu(), torch.from_numpy(ref.P6).float()) and torch.equal(m.basis_color_origin, m.basis_color.detach())
    # the guide at the bin centres is the table's rows (grid_sample with align_corners: exactly on the nodes up to fp32 rounding of the grid)
    centres = torch.from_numpy(extract.bin_centers_of(5)).to(cuda)
    guide = palette_utils.get_palette_weight_with_hist((centres * 32 - 0.5) / 31, hw)
    rows = lut[0].reshape(6, -1).t()
    assert guide.shape == rows.shape and float((guide - rows).abs().max()) < 2e-5
    # the same LUT through the old numpy entrance: one training batch gives the same weight guide, bit for bit
    old = small_model(cuda, 6)
    old.initialize_palette(ref.P6, hist_weights=extract.lut_to_hist_weights(lut))
    old = old.to(cuda)
    assert torch.equal(old.hist_weights.data, hw.data) and not old.hist_weights.is_contiguous()
    rng = np.random.default_rng(5)
    images = rng.random((2, 8, 8, 3)).astype(np.float32)
    poses = np.stack([np.eye(4, dtype=np.float32)] * 2)
    poses[:, 2, 3] = 1.5
    from palettenerf_amd import scene
    ts = trainset.TrainSet(images, poses, scene.intrinsics_from_fov(8, 8, 0.9), 8, 8, 64, device=cuda)
    torch.manual_seed(9)
    b_new = ts.batch(1, m)
    torch.manual_seed(9)
    b_old = ts.batch(1, old)
    assert b_new.gt_weights is not None and b_new.gt_weights.shape == (1, 64, 6)
    assert torch.equal(b_new.inds, b_old.inds) and torch.equal(b_new.gt_rgb, b_old.gt_rgb) and torch.equal(b_new.gt_weights, b_old.gt_weights)
    assert float((b_new.gt_weights.sum(dim=-1) - 1).abs().max()) < 1e-5
