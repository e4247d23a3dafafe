"""GPU: every compiled variant of the grid encoder -- k_grid_fwd<T, D, C>, k_grid_bwd<T, D, C, COMBINE> and k_grid_input_bwd<T> for T in {float, half},
D in 1..5, C in {1, 2, 4, 8} -- through the public grid_encode, against the float64 statement of tests/grid_reference.py (bounds derived there from the
precision of the number formats) and, where the oracle has the path, bit for bit against the oracle.

One test per (D, C); inside it gridtype x align_corners x table dtype, on the encoder's own offsets, on tiny tables for D <= 2 (so that hashed levels
occur) and on hand-made odd level sizes.  L = 6, H = 16, per_level_scale = 2: levels 0-4 run the run-combining backward kernel, level 5 the plain one.
The ray-ordered input (999 rows: runs of 2-27 equal table rows anywhere in a wave, out-of-range rows inside runs, a ragged last wave) is what the
segmented wave sum of k_grid_bwd<..., true> needs to be checked: a scan that drops or doubles one addend at a run boundary is far outside the bounds.

Every test prints its worst error / bound ratio per dtype and quantity (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import gridencoder
from palettenerf_amd._torch_glue import call, ptr
from tests import grid_reference as gr

pytestmark = pytest.mark.gpu

L, H, PLS = gr.L, gr.H, gr.PLS


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


class _Checks:
    """Collects every miss of one test (so that one run shows them all) and the worst error / bound ratio per (dtype, quantity)."""

    def __init__(self):
        self.fails, self.worst, self.cells = [], {}, 0

    def bound(self, tag, dtype, what, got, want, bound):
        r = gr.error_ratio(got, want, bound)
        if not r <= self.worst.get((dtype, what), 0.0):      # also when r is NaN
            self.worst[(dtype, what)] = r
        if not r <= 1.0:
            self.fails.append(f"{tag} {dtype} {what}: error / bound = {r}")

    def same_bits(self, tag, what, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(got.view(bits), want.view(bits)):
            self.fails.append(f"{tag} {what}: bits differ")

    def true(self, tag, what, ok):
        if not ok:
            self.fails.append(f"{tag} {what}")


def _encode(x, table, offsets, gridtype, ac, calc_grad_inputs=False):
    return gridencoder.grid_encode(x, table, offsets, PLS, H, calc_grad_inputs, gridtype, ac)


# what one table is walked through; tests/test_gpu_reference_grid.py walks the reference's own kernel through the same
QUANTITIES = ("forward", "forward with dy_dx", "dy_dx", "table gradient with input gradients", "table gradient without input gradients", "input gradient")
FORWARD_QUANTITIES = QUANTITIES[:3]


def run_table(encode, cuda, x, table, offsets, gridtype, ac, g, backward=True):
    """{quantity: numpy array} of `encode` (the signature of _encode) for one table: forward (without and with dy_dx), dy_dx as the autograd function
    saved it, and with `backward` the table gradient (with and without input gradients) and the input gradient.  "_out": the first forward's tensor."""
    tx, to = dev(x, cuda), dev(offsets, cuda)
    out = encode(tx, dev(table, cuda), to, gridtype, ac)
    te, txg = dev(table, cuda).requires_grad_(True), dev(x, cuda).requires_grad_(True)
    out2 = encode(txg, te, to, gridtype, ac, True)
    q = {"_out": out, "forward": host(out), "forward with dy_dx": host(out2), "dy_dx": host(out2.grad_fn.saved_tensors[3])}
    if backward:
        (out2 * dev(g, cuda)).sum().backward()
        te2 = dev(table, cuda).requires_grad_(True)
        (encode(tx, te2, to, gridtype, ac) * dev(g, cuda)).sum().backward()
        q["table gradient with input gradients"], q["table gradient without input gradients"] = host(te.grad), host(te2.grad)
        q["input gradient"] = host(txg.grad)
    return q


def want_table(ref, table, g, sparse=False):
    """The float64 values and magnitudes of one table, computed once for every subject that is held to them (sparse: the table gradient by way of
    GridReference.table_grad_sparse, for a table of millions of rows; the same values)."""
    w = {"forward": ref.forward(table), "dy_dx": ref.dy_dx(table), "table gradient": ref.table_grad_from_sparse(g) if sparse else ref.table_grad(g)}
    w["input gradient"] = ref.input_grad(g, *w["dy_dx"])
    return w


def check_table(ck, tag, dtype, ref, x, table, offsets, gridtype, ac, g, D, C, q, want=None, oracle_per_level_scale=PLS, oracle_base=H):
    """Holds the quantities of run_table to float64 (bounds of tests/grid_reference.py) and, for the forward, bit for bit to the oracle when
    `oracle_per_level_scale` is given.  ck.cells counts the quantities checked."""
    B, L_ = x.shape[0], ref.L
    u = gr.U32 if dtype == "fp32" else gr.U16
    w = want if want is not None else want_table(ref, table, g)
    out = q["forward"]
    fwd, mag = w["forward"]
    ck.true(tag, f"{dtype} output shape / dtype", out.shape == (B, L_ * C) and out.dtype == table.dtype)
    if oracle_per_level_scale is not None:
        ck.same_bits(tag, f"{dtype} forward against the oracle", out,
                     oracle.grid_encode_forward(x, table, offsets, oracle_per_level_scale, oracle_base, gridtype=gridtype, align_corners=ac))
    ck.bound(tag, dtype, "forward", out.reshape(B, L_, C), fwd, gr.forward_bound(D, mag, u))
    ck.true(tag, f"{dtype} out-of-range rows give zeros", not out[~ref.inr].any())
    ck.cells += 1

    # with dy_dx, then backward through the autograd wrapper
    ck.same_bits(tag, f"{dtype} forward with dy_dx requested", q["forward with dy_dx"], out)
    ck.cells += 1
    dy_gpu = q["dy_dx"].reshape(B, L_, D, C)
    dy, dmag = w["dy_dx"]
    ck.true(tag, f"{dtype} dy_dx dtype", dy_gpu.dtype == table.dtype)
    ck.bound(tag, dtype, "dy_dx", dy_gpu, dy, gr.dy_dx_bound(D, dmag) if dtype == "fp32" else gr.input_grad_bound(D, L_, C, dmag, u))
    ck.true(tag, f"{dtype} out-of-range rows give zero dy_dx", not dy_gpu[~ref.inr].any())
    ck.cells += 1
    if "input gradient" not in q:
        return
    gt, gmag, n = w["table gradient"]
    gbound = gr.table_grad_bound(D, gmag, n, u)
    wi, imag = w["input gradient"]
    touched = n > 0      # the bound is 0 on every other row (no addend: sum |w g| = 0), which asks for the exact zeros of the line after it
    gt_t, gbound_t = gt[touched], gbound[touched]
    for label in ("with input gradients", "without input gradients"):
        got = q[f"table gradient {label}"]
        ck.true(tag, f"{dtype} table gradient dtype {label}", got.dtype == table.dtype and got.shape == table.shape)
        ck.bound(tag, dtype, "table gradient", got[touched], gt_t, gbound_t)
        ck.true(tag, f"{dtype} untouched rows are exactly 0 {label}", not got[~touched].any())
        r = abs(got.astype(np.float64).sum() - gt.sum()) / gbound.sum()
        ck.true(tag, f"{dtype} checksum of the table gradient {label}: error / summed bound = {r}", r <= 1.0)
        ck.cells += 1
    gi = q["input gradient"]
    ck.true(tag, f"{dtype} input gradient dtype", gi.dtype == np.float32 and gi.shape == x.shape)
    ck.bound(tag, dtype, "input gradient", gi, wi, gr.input_grad_bound(D, L_, C, imag, u))
    ck.true(tag, f"{dtype} out-of-range rows get exactly 0 input gradient", not gi[~ref.inr].any())
    ck.cells += 1


def _one_table(ck, cuda, tag, dtype, ref, x, table, offsets, gridtype, ac, g, D, C):
    """forward (without and with dy_dx), backward (with and without input gradients) of one table dtype against float64."""
    q = run_table(_encode, cuda, x, table, offsets, gridtype, ac, g)
    check_table(ck, tag, dtype, ref, x, table, offsets, gridtype, ac, g, D, C, q)
    return q["_out"]


@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
def test_grid_variant_against_float64_and_the_oracle(cuda, D, C):
    ck = _Checks()
    for ci, (name, offsets, gridtype, ac) in enumerate(gr.variant_cases(D)):
        emb, g999 = gr.variant_tables(D, C, ci)
        emb16 = emb.astype(np.float16)
        for xname, x in gr.variant_inputs(D).items():
            tag = f"D{D} C{C} {name} {xname}"
            ref = gr.variant_geometry(D, ci, xname)
            g = g999[: x.shape[0]]
            out32 = _one_table(ck, cuda, tag, "fp32", ref, x, emb, offsets, gridtype, ac, g, D, C)
            out16 = _one_table(ck, cuda, tag, "fp16", ref, x, emb16, offsets, gridtype, ac, (g * 0.01).astype(np.float16), D, C)   # 0.01: nothing overflows half
            # autocast: an fp32 parameter goes to a half table when C is even (the packed-half atomics need pairs); C = 1 stays fp32
            with torch.autocast("cuda", dtype=torch.float16):
                auto = _encode(dev(x, cuda), dev(emb, cuda), dev(offsets, cuda), gridtype, ac)
            ck.same_bits(tag, "autocast forward", host(auto), host(out16 if C % 2 == 0 else out32))
    for (dtype, what), r in sorted(ck.worst.items()):
        print(f"grid variants D={D} C={C} {dtype} {what}: worst error / bound = {r:.3f}")
    assert not ck.fails, "\n".join(ck.fails)


@pytest.mark.parametrize("nt", [1, 2, 3])
def test_grid_d3c2_non_temporal_forms_against_float64_and_the_oracle(cuda, nt):
    """pnr_set_option("grid_nt", 1 | 2 | 3) sends the D = 3, C = 2 forward to k_grid_fwd_d3c2<T, false, NT> (non-temporal output stores, input loads,
    both): other instructions for the same arithmetic, so the checks of the (3, 2) case above hold unchanged, for both table types."""
    from palettenerf_amd import _lib
    lib = _lib.load()
    D, C = 3, 2
    ck = _Checks()
    try:
        assert lib.pnr_set_option(b"grid_nt", nt) == 0
        for ci, (name, offsets, gridtype, ac) in enumerate(gr.variant_cases(D)):
            emb, g999 = gr.variant_tables(D, C, ci)
            for xname, x in gr.variant_inputs(D).items():
                tag = f"nt{nt} {name} {xname}"
                ref = gr.variant_geometry(D, ci, xname)
                g = g999[: x.shape[0]]
                _one_table(ck, cuda, tag, "fp32", ref, x, emb, offsets, gridtype, ac, g, D, C)
                _one_table(ck, cuda, tag, "fp16", ref, x, emb.astype(np.float16), offsets, gridtype, ac, (g * 0.01).astype(np.float16), D, C)
    finally:
        lib.pnr_set_option(b"grid_nt", 0)
    assert not ck.fails, "\n".join(ck.fails)


@pytest.mark.parametrize("D,C,levels", [(6, 2, 4), (3, 3, 4), (3, 2, 33)])
def test_grid_unsupported_shapes_raise_forward_and_backward(cuda, D, C, levels):
    """D = 6, C = 3 and L = 33 are not compiled: RuntimeError `unsupported` from the forward (through grid_encode) and from the backward entry point
    (the wrapper cannot reach it without a forward, so through the C ABI); nothing is launched and the gradient buffers stay as they were."""
    B, rows = 16, 64
    x = torch.rand(B, D, device=cuda)
    offsets = torch.arange(levels + 1, dtype=torch.int32, device=cuda) * rows
    for dtype_id, dtype in ((0, torch.float32), (1, torch.float16)):
        table = torch.rand(rows * levels, C, device=cuda).to(dtype)
        with pytest.raises(RuntimeError, match="unsupported"):
            gridencoder.grid_encode(x, table, offsets, 2.0, 4, False, 0, False)
        with pytest.raises(RuntimeError, match="unsupported"):
            gridencoder.grid_encode(x, table, offsets, 2.0, 4, True, 0, False)
        grad = torch.ones(levels, B, C, device=cuda, dtype=dtype)
        gg, dy_dx, gi = torch.zeros_like(table), torch.zeros(B, levels * D * C, device=cuda, dtype=dtype), torch.zeros(B, D, device=cuda, dtype=dtype)
        for with_inputs in (False, True):
            with pytest.raises(RuntimeError, match="unsupported"):
                call("pnr_grid_encode_backward", ptr(grad), ptr(x), ptr(table), ptr(offsets), ptr(gg), B, D, C, levels, 1.0, 4,
                     ptr(dy_dx) if with_inputs else None, ptr(gi) if with_inputs else None, 0, 0, dtype_id)
        assert not gg.any() and not gi.any()
