"""The REFERENCE'S OWN hash-grid kernels (gridencoder.cu: kernel_grid, kernel_grid_backward, kernel_input_backward) executed on the MI355X, as a second
subject of the checks tests/test_gpu_grid_variants.py holds this repository's kernels to.

oracle/_ref/ref_gridencoder.so is gridencoder.cu + bindings.cpp of the reference compiled for gfx950 (oracle/ref_build.py: build_hip), called through
oracle/ref_ops.py: grid_encode, which restates the few lines gridencoder/grid.py puts around `_backend`.  The source is unmodified; the one overload
the HIP headers lack, atomicAdd(__half2*, __half2), is this repository's stand-in on unsafeAtomicAdd (oracle/ref_half2_atomic.h).  It is reached
only by the table gradient of an fp16 table with an even feature count: there the accumulation primitive is this repository's, everything else --
forward, dy_dx, input gradient, the whole fp32 path -- is the reference's code on the reference's calls.

(a) their kernel against the float64 statement of tests/grid_reference.py over the whole variant matrix: the test of OUR READING of gridencoder.cu
    (dense / hash switch, the `%` wrap, what is out of range, scale and resolution of a level, the order of dy_dx, which samples scatter), with the
    bounds derived there and no margin.  ONE exclusion: the backward of an fp16 table with C = 1 -- the reference has no such path (its
    atomicAdd(at::Half*, at::Half), gridencoder.cu:22-26, is an empty function, and grid.py:38 never makes a half table for odd C); the forward
    and dy_dx of that table are checked.  The cells run are counted and the count is held to the number computed from the matrix.
(b) ours against theirs on the same cells: the number of elements whose bits differ, per (D, C, dtype, quantity), printed (pytest -s) and recorded
    in profiles/reference_grid/README.md; what showed no differing element in any case is asserted bit-identical (bit_identical): dy_dx, and the
    forward but for fp32 D = 1 C = 1 and fp16 C = 1.
(c) the shipped geometry (the encoder palettenerf_amd/network.py builds for the NeRF field: fine levels, wrapped strides, large hashed
    coordinates -- what the L = 6 matrix never reaches), both kernels against float64.
(d) one frame of scene S0 under all four reference kernel families against the same frame under this repository's kernels.

A missing ref_gridencoder.so FAILS these tests; it never skips them."""
import functools

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import gridencoder, raymarching, scene
from tests import grid_reference as gr
from tests.test_gpu_grid_variants import FORWARD_QUANTITIES, QUANTITIES, _Checks, check_table, run_table, want_table
from tests.test_gpu_reference_kernels import FRAME_ATOL

pytestmark = pytest.mark.gpu

# What the first run of both kernels on the MI355X showed (profiles/reference_grid/README.md), asserted from then on.  Between this repository's kernel
# and the reference's no element differed in bits, in any cell of the variant matrix or on the shipped geometry, for dy_dx (every dtype, D, C) and for
# the forward, without and with dy_dx -- but for the (dtype, D, C) of FORWARD_DIFFERS, where the VALUES of some elements differ because the compiler
# selected other instructions for those instantiations of the reference's kernel (read from the disassembly of the built module, README section (b)):
#   fp32, D = 1, C = 1 (16 267 of 67 824 elements): the two corner products of the accumulation at gridencoder.cu:165 became one packed multiply and
#     two adds -- each product rounded, then the sum -- where every other instantiation, this repository's kernel and the oracle chain fused
#     multiply-adds (one rounding per corner);
#   fp16, C = 1, every D (2-6 elements each): the product is rounded ONCE to half by a mixed-precision fma, where every other instantiation, this
#     repository's kernel and the oracle round it to fp32 and then to half.
# The oracle's forward against the reference kernel's forward: the same picture.  The table gradient (atomics in any order) and the input gradient
# (another order of the L C terms) differ in bits, as expected.  For these, and for the forward of FORWARD_DIFFERS, the float64 bound on each side is
# the assertion.
FORWARD_DIFFERS = {("fp32", 1, 1)} | {("fp16", D, 1) for D in (1, 2, 3, 4, 5)}


def bit_identical(dtype, what, D, C):
    """whether `what` of a (dtype, D, C) is held to bit-identity with the reference's kernel ("oracle forward": the oracle's forward with theirs)"""
    return what == "dy_dx" or (what in ("forward", "forward with dy_dx", "oracle forward") and (dtype, D, C) not in FORWARD_DIFFERS)


@pytest.fixture(scope="module")
def ref_grid(cuda):
    from oracle import ref_build, ref_ops
    if not ref_ops.grid_available():
        pytest.fail("oracle/_ref/ref_gridencoder.so is not built (oracle/ref_build.py: build_hip compiles it where the reference checkout is; "
                    "__graft_entry__.build() calls it).  The reference's hash-grid kernel is this file's subject: nothing here can run without it")
    be = ref_build.load_hip("gridencoder")
    assert hasattr(be, "grid_encode_forward") and hasattr(be, "grid_encode_backward")
    print(f"ref_gridencoder.so: built {ref_build.hip_build_note('gridencoder')}")
    return ref_ops


def _differ(a, b):
    """(elements whose bits differ, elements whose values differ): the first counts a -0.0 against a +0.0, the second does not"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    bits = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return np.array([(a.view(bits) != b.view(bits)).sum(), (a != b).sum()], np.int64)


def _tally(diff, key, elements, differing):
    e, d = diff.get(key, (0, np.zeros(2, np.int64)))
    diff[key] = (e + elements, d + differing)


def matrix_cells(D, C):
    """(D, C, case, input, dtype, quantity) cells of one (D, C): every quantity for the fp32 table, and for the fp16 table unless C = 1 (forward ones only)"""
    return len(gr.variant_cases(D)) * len(gr.variant_inputs(D)) * (len(QUANTITIES) + (len(FORWARD_QUANTITIES) if C == 1 else len(QUANTITIES)))


def _report(title, ck_ref, ck_ours, diff):
    for (dtype, what), r in sorted(ck_ref.worst.items()):
        print(f"{title} | {dtype} | {what} | worst error / bound: reference {r:.3f} ours {ck_ours.worst.get((dtype, what), float('nan')):.3f}")
    for (dtype, what), (elements, differing) in sorted(diff.items()):
        print(f"{title} | {dtype} | {what} | elements {elements} | bits differ {differing[0]} | values differ {differing[1]}")


@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
def test_reference_grid_kernel_against_float64_and_ours_over_the_variant_matrix(cuda, ref_grid, D, C):
    def theirs_encode(x, table, offsets, gridtype, ac, calc_grad_inputs=False):
        return ref_grid.grid_encode(x, table, offsets, gr.PLS, gr.H, calc_grad_inputs, gridtype, ac)

    def ours_encode(x, table, offsets, gridtype, ac, calc_grad_inputs=False):
        return gridencoder.grid_encode(x, table, offsets, gr.PLS, gr.H, calc_grad_inputs, gridtype, ac)

    ck_ref, ck_ours, diff = _Checks(), _Checks(), {}
    for ci, (name, offsets, gridtype, ac) in enumerate(gr.variant_cases(D)):
        emb, g999 = gr.variant_tables(D, C, ci)
        for xname, x in gr.variant_inputs(D).items():
            tag = f"D{D} C{C} {name} {xname}"
            ref = gr.variant_geometry(D, ci, xname)
            g32 = g999[: x.shape[0]]
            for dtype, table, g in (("fp32", emb, g32), ("fp16", emb.astype(np.float16), (g32 * 0.01).astype(np.float16))):   # 0.01: nothing overflows half
                backward = not (dtype == "fp16" and C == 1)       # THE exclusion: the reference has no backward for a half table with C = 1
                want = want_table(ref, table, g)
                theirs = run_table(theirs_encode, cuda, x, table, offsets, gridtype, ac, g, backward=backward)
                check_table(ck_ref, "reference " + tag, dtype, ref, x, table, offsets, gridtype, ac, g, D, C, theirs, want, oracle_per_level_scale=None)
                ours = run_table(ours_encode, cuda, x, table, offsets, gridtype, ac, g)
                check_table(ck_ours, "ours " + tag, dtype, ref, x, table, offsets, gridtype, ac, g, D, C, ours, want, oracle_per_level_scale=None)
                for what in (QUANTITIES if backward else FORWARD_QUANTITIES):
                    n = _differ(ours[what], theirs[what])
                    _tally(diff, (dtype, what), theirs[what].size, n)
                    if bit_identical(dtype, what, D, C):
                        ck_ref.true(tag, f"{dtype} {what}: {n[0]} elements differ in bits between ours and the reference's kernel", n[0] == 0)
                n = _differ(oracle.grid_encode_forward(x, table, offsets, gr.PLS, gr.H, gridtype=gridtype, align_corners=ac), theirs["forward"])
                _tally(diff, (dtype, "oracle forward"), theirs["forward"].size, n)
                if bit_identical(dtype, "oracle forward", D, C):
                    ck_ref.true(tag, f"{dtype} forward: {n[0]} elements differ in bits between the oracle and the reference's kernel", n[0] == 0)
    _report(f"reference grid D={D} C={C}", ck_ref, ck_ours, diff)
    assert not (ck_ref.fails or ck_ours.fails), "\n".join(ck_ref.fails + ck_ours.fails)
    assert ck_ref.cells == matrix_cells(D, C), f"ran {ck_ref.cells} cells of the reference's kernel, the matrix has {matrix_cells(D, C)}"


def test_matrix_cell_count():
    """The number the test above holds its count to, written out: 5 or 9 cases x 2 inputs x (6 + 6 quantities, 6 + 3 for C = 1)."""
    assert [len(gr.variant_cases(D)) for D in (1, 2, 3, 4, 5)] == [9, 9, 5, 5, 5] and len(gr.variant_inputs(3)) == 2 and len(QUANTITIES) == 6
    assert sum(matrix_cells(D, C) for D in (1, 2, 3, 4, 5) for C in (1, 2, 4, 8)) == 33 * 2 * (9 + 3 * 12)


# ------------------------------------------------------------------------------------------ (c) the shipped geometry
def shipped_encoder():
    """The encoder of the NeRF field as palettenerf_amd/network.py builds it (bound = 1)."""
    from palettenerf_amd import network
    enc = network.NeRFNetwork(bound=1, cuda_ray=True).encoder
    assert (enc.input_dim, enc.level_dim, enc.num_levels, enc.base_resolution, enc.log2_hashmap_size) == (3, 2, 16, 16, 19)
    assert enc.gridtype_id == 0 and not enc.align_corners and abs(enc.base_resolution * enc.per_level_scale ** 15 - 2048) < 1e-6
    return enc


@functools.lru_cache(maxsize=None)
def shipped_inputs():
    """[4112, 3] float32: 4096 ray-ordered points (151 segments of 27 samples + 19 loose ones) and the boundary rows of variant_inputs(3)"""
    rng = np.random.default_rng(4096)
    start = rng.random((151, 1, 3)) * 0.9
    step = (0.1 / 27) * (0.5 + 0.5 * rng.random((151, 1, 3)))
    rays = np.concatenate([(start + np.arange(27)[None, :, None] * step).reshape(4077, 3), rng.random((19, 3))]).astype(np.float32)
    v = gr.variant_inputs(3)["rays"]
    x = np.concatenate([rays, v[[100, 200, 400, 401, 500, 600]], v[300:310]])
    assert rays.shape == (4096, 3) and rays.min() >= 0 and rays.max() < 1 and x.shape == (4112, 3)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def shipped_geometry():
    enc = shipped_encoder()
    offsets = enc.offsets.numpy().copy()
    return offsets, float(enc.per_level_scale), gr.GridReference(shipped_inputs(), offsets, float(enc.per_level_scale), 16, 0, False)


@pytest.mark.parametrize("amplitude", [1e-4, 0.5])
def test_shipped_geometry_both_kernels_against_float64(cuda, ref_grid, amplitude):
    """D = 3, C = 2, 16 levels from 16 to 2048, 2^19 rows per hashed level; table values U(-1e-4, 1e-4) (the reference's init, grid.py:131-133) and
    U(-0.5, 0.5); fp32 and fp16 tables.  The table gradient is dense in the table: the bound is 0 on the rows no sample touches, so they have to
    be exact zeros."""
    offsets, pls, ref = shipped_geometry()
    x = shipped_inputs().copy()      # the shared array is read-only
    D, C, L_ = 3, 2, 16
    rng = np.random.default_rng(int(amplitude * 1e6))
    emb = ((rng.random((int(offsets[-1]), C)) - 0.5) * 2 * amplitude).astype(np.float32)
    g32 = rng.standard_normal((x.shape[0], L_ * C)).astype(np.float32)

    def theirs_encode(x, table, offsets, gridtype, ac, calc_grad_inputs=False):
        return ref_grid.grid_encode(x, table, offsets, pls, 16, calc_grad_inputs, gridtype, ac)

    def ours_encode(x, table, offsets, gridtype, ac, calc_grad_inputs=False):
        return gridencoder.grid_encode(x, table, offsets, pls, 16, calc_grad_inputs, gridtype, ac)

    ck_ref, ck_ours, diff = _Checks(), _Checks(), {}
    for dtype, table, g in (("fp32", emb, g32), ("fp16", emb.astype(np.float16), (g32 * 0.01).astype(np.float16))):
        want = want_table(ref, table, g, sparse=True)     # 6.1 million rows, some 300 000 of them touched
        assert (want["table gradient"][2] == 0).sum() > 1_000_000 and (want["table gradient"][2] > 0).sum() > 100_000
        theirs = run_table(theirs_encode, cuda, x, table, offsets, 0, False, g)
        check_table(ck_ref, f"reference shipped {amplitude}", dtype, ref, x, table, offsets, 0, False, g, D, C, theirs, want, oracle_per_level_scale=None)
        ours = run_table(ours_encode, cuda, x, table, offsets, 0, False, g)
        check_table(ck_ours, f"ours shipped {amplitude}", dtype, ref, x, table, offsets, 0, False, g, D, C, ours, want, oracle_per_level_scale=pls, oracle_base=16)
        for what in QUANTITIES:
            n = _differ(ours[what], theirs[what])
            _tally(diff, (dtype, what), theirs[what].size, n)
            if bit_identical(dtype, what, D, C):      # D = 3, C = 2: forward and dy_dx, as in the matrix
                ck_ref.true(f"shipped {amplitude}", f"{dtype} {what}: {n[0]} elements differ in bits between ours and the reference's kernel", n[0] == 0)
    _report(f"reference grid shipped amplitude={amplitude}", ck_ref, ck_ours, diff)
    assert not (ck_ref.fails or ck_ours.fails), "\n".join(ck_ref.fails + ck_ours.fails)
    assert ck_ref.cells == ck_ours.cells == 2 * len(QUANTITIES)


# ------------------------------------------------------------------------------------------ (d) one frame under all four reference kernel families
def test_frame_under_all_four_reference_kernel_families_equals_the_frame_under_ours(cuda, ref_grid):
    """A 64 x 64 window of the 800 x 800 frame of scene S0 through the per-op loop, once over this repository's kernels and once with the reference's
    march, composite, SH AND hash-grid kernels swapped in: the same samples, and images within the tolerance the three-family swap is held to
    (tests/test_gpu_reference_kernels.py: FRAME_ATOL)."""
    from oracle import ref_ops
    from palettenerf_amd import network
    if not ref_ops.available():
        pytest.fail("oracle/_ref/ref_{raymarching,shencoder,palette}.so are not built (oracle/ref_build.py: build_hip)")
    H = W = 800
    ro, rd = scene.get_rays(torch.from_numpy(scene.lookat_pose())[None], scene.intrinsics_from_fov(H, W), H, W)
    rows = (torch.arange(368, 432)[:, None] * W + torch.arange(368, 432)[None, :]).reshape(-1)
    ro, rd = ro[:, rows].contiguous().to(cuda), rd[:, rows].contiguous().to(cuda)

    def frame():
        m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1.0, min_near=0.2)
        scene.seed_field_(m, 0)
        m = m.to(cuda).eval()
        m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
        m.density_bitfield.copy_(raymarching.packbits(m.density_grid, 0.5))
        m.count_rendered = True
        with torch.no_grad():
            return m.render(ro, rd, perturb=False, dt_gamma=0.0, max_steps=1024, T_thresh=1e-4)

    ours = frame()
    calls = ref_ops.grid_encode.calls
    with ref_ops.swapped_in(grid=True):
        theirs = frame()
    assert ref_ops.grid_encode.calls > calls, "the frame under swapped_in(grid=True) never called the reference's grid kernel"
    assert gridencoder.grid_encode is not ref_ops.grid_encode
    assert int(ours["rendered"].sum()) == int(theirs["rendered"].sum()) > 4096
    worst = float((ours["image"] - theirs["image"]).abs().max())
    print(f"reference grid frame | samples {int(ours['rendered'].sum())} | max |image difference| {worst:.3e}")
    assert worst <= FRAME_ATOL
    assert torch.equal(ours["weights_sum"] > 0, theirs["weights_sum"] > 0)
