"""The bucket-binned hash-grid table gradient (csrc/grid_binned.hip: pnr_grid_encode_backward_binned; D = 3, C = 2, fp32 tables -- the table gradient of
every training step) in every regime, against the float64 statement of tests/grid_reference.py and its derived bound (n + D + 3) u S per element.

Per level the host picks one of four treatments -- fp64 LDS images (k_coarse_image / k_coarse_reduce), records of runs of equal rows (COMBINE = 1), records
of runs of samples in one cell (COMBINE = 2), a record per sample and corner (COMBINE = 0) -- and one of two scatter kernels; a gather job owns its bucket
or shares it (global atomics).  Geometry A has all four treatments on the encoder's own offsets (hash / tiled, align_corners off / on), geometry B
hand-made level sizes (a dense level inside a larger allocation, hashed levels of no power-of-two size over several buckets, last buckets of one row, a
9-bucket level), geometry C a bucket crowded enough to be split into two jobs.  Each runs under six option sets that move levels from one treatment to
another.  The inputs are ray-ordered (runs that start and end anywhere in a wave and in a row of 16 lanes) and the output gradient has what a real
batch has: exact zeros behind each ray's stopping sample and scattered among the live samples (drop_dead), samples with one zero channel, -0.0.

The non-staged scatter (k_bin_scatter<0/1/2>) is what the host takes by itself when the staged kernel's LDS would exceed 160 KiB: more than ~5460
buckets, a table of ~45 M rows -- too large for a quick test.  The same kernels run here through the option scatter_staged = 0.

The staged scatter's dynamic LDS grows with the table (its per-bucket counters: 12 bytes per possible bucket), and a kernel's dynamic-LDS limit is
raised once per process and device: test_binned_small_table_then_a_larger_one_in_a_fresh_process runs a small table first and a larger one after it.

Every GPU test prints its worst error / bound ratio per case and option set (pytest -s shows them).  The last test needs no device: it checks that the
constructions above are what they claim to be, that the fp32 oracle stays inside the bound on them and that a gradient lacking one sample does not."""
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import _lib, gridencoder
from palettenerf_amd._torch_glue import ptr, stream_ptr
from tests import grid_reference as gr

OPTION_SETS = ((), ("coarse_image",), ("cell_merge",), ("scatter_staged",), ("coarse_image", "scatter_staged"), ("cell_merge", "scatter_staged"))   # switched OFF
PNR_ERR_INVALID = -1


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)       # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def _label(off):
    return " + ".join(f"{o}=0" for o in off) or "default"


@contextmanager
def _options_off(off):
    lib = _lib.load()
    try:
        for o in off:
            assert lib.pnr_set_option(o.encode(), 0) == 0
        yield
    finally:
        for o in ("coarse_image", "cell_merge", "scatter_staged"):
            lib.pnr_set_option(o.encode(), 1)


def _check(fails, tag, got, want, bound, n, before=None):
    """the four checks of test_gpu_grid_variants._one_table on one table gradient; -> error / bound"""
    got64 = got.astype(np.float64) - (0.0 if before is None else before.astype(np.float64))
    r = gr.error_ratio(got64, want, bound)
    if not r <= 1.0:
        fails.append(f"{tag}: error / bound = {r}")
    untouched = got[n == 0] if before is None else (got[n == 0] - before[n == 0])
    if untouched.any():
        fails.append(f"{tag}: {np.count_nonzero(untouched.any(axis=1))} rows that no sample reaches changed")
    s = abs(got64.sum() - want.sum()) / bound.sum()
    if not s <= 1.0:
        fails.append(f"{tag}: checksum error / summed bound = {s}")
    if got.dtype != np.float32 or got.shape != want.shape:
        fails.append(f"{tag}: dtype / shape {got.dtype} {got.shape}")
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", gr.BINNED_CASES)
def test_binned_table_gradient_against_float64(cuda, name, monkeypatch):
    """grid_encode(...).backward on the binned path, six option sets against one float64 reference"""
    L, H, pls, offsets, gridtype, ac = gr.binned_case(name)
    x, g = gr.binned_inputs(name), gr.binned_grad(name)
    _, gt, mag, n = gr.binned_reference(name)
    bound = gr.table_grad_bound(3, mag, n)
    monkeypatch.setattr(gridencoder, "BINNED_MIN_ROWS", 1)
    entries, real_call = [], gridencoder.call

    def spy(entry, *a, **k):                                   # which entry point the autograd wrapper took
        entries.append(entry)
        return real_call(entry, *a, **k)
    monkeypatch.setattr(gridencoder, "call", spy)
    tx, to, tg = dev(x, cuda), dev(offsets, cuda), dev(g, cuda)
    rows = int(offsets[-1])
    fails = []
    for off in OPTION_SETS:
        with _options_off(off):
            te = torch.zeros(rows, 2, device=cuda).requires_grad_(True)
            (gridencoder.grid_encode(tx, te, to, pls, H, False, gridtype, ac) * tg).sum().backward()
            got = host(te.grad)
        r = _check(fails, f"{name} {_label(off)}", got, gt, bound, n)
        print(f"binned table gradient {name} [{_label(off)}]: worst error / bound = {r:.3f}")
    assert entries.count("pnr_grid_encode_backward_binned") == len(OPTION_SETS) and "pnr_grid_encode_backward" not in entries
    assert not fails, "\n".join(fails)


def _abi(cuda, name, x, g, out, short=0, rows_used=None):
    """pnr_grid_encode_backward_binned straight through the C ABI, adding into `out` (a device tensor); -> the return code"""
    return _abi_case(cuda, gr.binned_case(name), x, g, out, short, rows_used)


def _abi_case(cuda, case, x, g, out, short=0, rows_used=None):
    L, H, pls, offsets, gridtype, ac = case
    lib = _lib.load()
    B = x.shape[0] if rows_used is None else rows_used
    rows = int(offsets[-1])
    nbytes = int(lib.pnr_grid_backward_binned_workspace_bytes(B, L, rows))
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=cuda)
    glm = dev(np.asarray(g).reshape(x.shape[0], L, 2).transpose(1, 0, 2), cuda)       # level-major, as the kernels take it
    tx, to = dev(x, cuda), dev(offsets, cuda)                                         # named: they have to outlive the call
    rc = lib.pnr_grid_encode_backward_binned(ptr(glm), ptr(tx), ptr(to), ptr(out), B, 3, 2, L, float(np.float32(np.log2(pls))), H,
                                             gridtype, int(ac), rows, ptr(ws), nbytes - short, stream_ptr())
    torch.cuda.synchronize()
    del glm, tx, to, ws
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 65, 1025])
def test_binned_small_and_ragged_batches_through_the_abi(cuda, B):
    """less than a wave, a wave +- 1, a workgroup + 1: the first B rows of geometry A; a workspace one byte short and B = 0 write nothing"""
    name = "A-hash"
    x, g = gr.binned_inputs(name)[:B], gr.binned_grad(name)[:B]
    _, gt, mag, n = gr.binned_reference(name, B)
    bound = gr.table_grad_bound(3, mag, n)
    rows = gt.shape[0]
    out = torch.zeros(rows, 2, device=cuda)
    assert _abi(cuda, name, x, g, out) == 0
    fails = []
    r = _check(fails, f"{name} B={B}", host(out), gt, bound, n)
    print(f"binned table gradient {name} B={B} [default]: worst error / bound = {r:.3f}")
    assert not fails, "\n".join(fails)
    pattern = torch.full((rows, 2), 0.75, device=cuda)
    assert _abi(cuda, name, x, g, pattern, short=1) == PNR_ERR_INVALID
    assert bool((pattern == 0.75).all())
    assert _abi(cuda, name, x, g, pattern, rows_used=0) == 0
    assert bool((pattern == 0.75).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A-hash", "C"])
def test_binned_adds_into_the_gradient_buffer(cuda, name):
    """the image reduce, the exclusive gather job and the split one (geometry C) all ADD: into a buffer that holds a pattern p, got - p is the gradient
    within the bound plus the one extra rounding u |p + gradient|; rows that no sample reaches keep p bit for bit"""
    x, g = gr.binned_inputs(name), gr.binned_grad(name)
    _, gt, mag, n = gr.binned_reference(name)
    # p: of the size of the row's own terms where addends arrive (0.25 ... 1 of sum |w g|, either sign: grid_reference.table_grad_accumulate_bound says
    # why no larger), ~3 on the rows that none reaches
    rng = np.random.default_rng(77)
    before = np.where(n[:, None] > 0, mag * rng.uniform(0.25, 1.0, gt.shape) * rng.choice([-1.0, 1.0], gt.shape), 3.0 * rng.standard_normal(gt.shape)).astype(np.float32)
    bound = gr.table_grad_accumulate_bound(3, mag, n, gt, before)
    fails = []
    for off in ((), ("coarse_image",)):
        with _options_off(off):
            out = dev(before, cuda)
            assert _abi(cuda, name, x, g, out) == 0
        r = _check(fails, f"{name} accumulate {_label(off)}", host(out), gt, bound, n, before)
        print(f"binned table gradient {name} added to a filled buffer [{_label(off)}]: worst error / bound = {r:.3f}")
    assert not fails, "\n".join(fails)


# (levels, rows per level), in the order of the calls: total rows / 8192 + L = 3 possible buckets, then 36 -- the staged scatter's LDS is 96 KiB + 12 bytes
# per possible bucket + 16, above the 64 KiB default either way, and larger for the second table.  H = 16, per_level_scale = 2: level 0 is an LDS image,
# the levels behind it go through the staged scatter (17^3 cells are hashed into 4096 rows and lie inside 65536; from 65^3 on both tables are hashed).
LDS_ORDER_TABLES = ((2, 4096), (4, 1 << 16))
LDS_ORDER_POINTS = 4096


def _small_table_then_a_larger_one():
    """(the child process) both table gradients through the ABI, each against the float64 reference and its bound; -> the exit status"""
    if not torch.cuda.is_available():
        print("no GPU is visible")
        return 2
    cuda = torch.device("cuda:0")
    fails = []
    for L, rows in LDS_ORDER_TABLES:
        offsets = (np.arange(L + 1) * rows).astype(np.int32)
        rng = np.random.default_rng(rows)
        x, g = rng.random((LDS_ORDER_POINTS, 3)).astype(np.float32), rng.standard_normal((LDS_ORDER_POINTS, L * 2)).astype(np.float32)
        gt, mag, n = gr.GridReference(x, offsets, 2.0, 16).table_grad(g)
        out = torch.zeros(L * rows, 2, device=cuda)
        tag = f"L = {L}, {rows} rows per level"
        rc = _abi_case(cuda, (L, 16, 2.0, offsets, 0, False), x, g, out)
        if rc != 0:
            fails.append(f"{tag}: pnr_grid_encode_backward_binned returned {rc}")
        r = _check(fails, tag, host(out), gt, gr.table_grad_bound(3, mag, n), n)
        print(f"binned table gradient, {tag}: return code {rc}, worst error / bound = {r:.3f}")
    print("\n".join(fails))
    return 1 if fails else 0


@pytest.mark.gpu
def test_binned_small_table_then_a_larger_one_in_a_fresh_process(cuda):
    """the dynamic-LDS limit of the staged scatter does not depend on which table a process brings first (a fresh process: the flags are process-wide)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "tests.test_gpu_grid_binned"], cwd=root, capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("worst error / bound") == len(LDS_ORDER_TABLES)


# ------------------------------------------------------------------------------------------ no device
def _runs(key, width):
    """maximal runs of equal consecutive keys (key < 0: never equal), cut every `width` samples -> (start, length) arrays"""
    i = np.arange(len(key))
    head = np.ones(len(key), bool)
    head[1:] = (key[1:] != key[:-1]) | (key[1:] < 0) | (i[1:] % width == 0)
    start = np.flatnonzero(head)
    return start, np.diff(np.append(start, len(key)))


def test_binned_constructions_are_what_they_claim():
    # level classification, recomputed with the host's rules
    L, H, pls, offsets, _, _ = gr.binned_case("A-hash")
    sizes, buckets, kinds = gr.binned_level_plan(L, pls, H, offsets, False)
    assert sizes == (4920, 15632, 50656) + (131072,) * 5 and buckets == (1, 2, 7) + (16,) * 5
    assert kinds == ("image", "image", 2, 2, 2, 2, 2, 0)
    assert gr.binned_level_plan(L, pls, H, offsets, False, coarse_image=False)[2] == (1, 1, 2, 2, 2, 2, 2, 0)
    assert gr.binned_level_plan(L, pls, H, offsets, False, cell_merge=False)[2] == ("image", "image", 0, 0, 0, 0, 0, 0)
    assert any(b <= 8 for b, k in zip(buckets, kinds) if k != "image") and any(b > 8 for b in buckets)     # aggregated and per-lane reservation
    ac_off = gr.binned_case("A-hash-ac")[3]
    sizes_ac, buckets_ac, kinds_ac = gr.binned_level_plan(L, pls, H, ac_off, True)
    assert sizes_ac[:3] == (16 ** 3, 24 ** 3, 36 ** 3) and kinds_ac == kinds and buckets_ac[1] == 2
    Lb, Hb, plsb, off_b, _, _ = gr.binned_case("B-hash")
    sizes_b, buckets_b, kinds_b = gr.binned_level_plan(Lb, plsb, Hb, off_b, False)
    assert sizes_b == gr.BINNED_B_SIZES and sum(sizes_b) % 2 == 0 and buckets_b == (1, 2, 2, 3, 4, 9) and kinds_b == ("image", 2, 2, 2, 2, 0)
    assert gr.binned_level_plan(Lb, plsb, Hb, off_b, False, coarse_image=False)[2] == (1, 2, 2, 2, 2, 0)
    _, res_b = oracle.grid_level_params(Lb, plsb, Hb)
    assert (int(res_b[0]) + 1) ** 3 < sizes_b[0]                                    # a dense level inside a larger allocation
    for l in (1, 3, 4, 5):                                                          # hashed, no power of two: the general row index
        assert (int(res_b[l]) + 1) ** 3 > sizes_b[l] and sizes_b[l] & (sizes_b[l] - 1)

    worst_oracle = {}
    for name in gr.BINNED_CASES:
        L, H, pls, offsets, gridtype, ac = gr.binned_case(name)
        x, g = gr.binned_inputs(name), gr.binned_grad(name)
        assert not x.flags.writeable and not g.flags.writeable and x.dtype == np.float32 and g.dtype == np.float32
        ref, gt, mag, n = gr.binned_reference(name)
        bound = gr.table_grad_bound(3, mag, n)
        live = gr.binned_live(ref, g)
        # the fp32 oracle's sequential scatter is inside the bound ...
        ogg = oracle.grid_encode_backward(g, x, (int(offsets[-1]), 2), offsets, pls, H, gridtype=gridtype, align_corners=ac)
        worst_oracle[name] = gr.error_ratio(ogg, gt, bound)
        assert worst_oracle[name] <= 1.0, (name, worst_oracle[name])
        # ... and a gradient that lacks one live sample on one level is not, on every level
        for l in range(L):
            cand = np.flatnonzero(live[l])
            sample = int(cand[len(cand) // 2])
            r = gr.deleted_sample_ratio(ref, g, bound, l, sample)
            assert r > 1.0, (name, l, sample, r)
        # ... nor one that lacks a sample altogether (every level recomputed)
        if name in ("A-hash", "C"):
            g2 = g.copy()
            sample = int(np.flatnonzero(live.all(axis=0))[7])
            g2[sample] = 0.0
            r = gr.error_ratio(ref.table_grad(g2)[0], gt, bound)
            print(f"{name}: float64 gradient without sample {sample}: error / bound = {r:.3g}")
            assert r > 1.0

        if name[0] == "B":      # every one-row last bucket is reached by a live sample
            assert x.shape[0] > gr.BINNED_RAYS
            one_row = [l for l in range(L) if sizes_b[l] % gr.BIN_ROWS == 1]
            assert one_row == [1, 3, 4]
            for l in one_row:
                hit = (ref.rows[l] == int(offsets[l + 1]) - 1).any(axis=0) & live[l]
                assert hit.any(), (name, l)
                assert n[int(offsets[l + 1]) - 1] > 0
        if name == "C":         # level 2: one bucket split between two gather jobs, whatever the cell merge removes; another in one piece
            rec = gr.binned_bucket_records(ref, g, offsets, 2)
            same_cell = (ref.rows[2, 0, 1:] == ref.rows[2, 0, :-1]) & live[2, 1:] & live[2, :-1] & (np.arange(1, ref.B) % 16 != 0)    # level 2 is dense: corner 0's row names the cell
            merged_away = 8 * int(same_cell.sum())
            assert rec.max() > gr.BIN_CHUNK and rec.max() - merged_away > gr.BIN_CHUNK, (rec, merged_away)
            assert rec.max() - merged_away <= 2 * gr.BIN_CHUNK
            assert ((rec >= 1) & (rec <= gr.BIN_CHUNK)).any(), rec
            # run-merged as COMBINE = 1 (coarse_image = 0), levels 0 and 1 are split as well: random order, nearly nothing merges
            assert gr.binned_bucket_records(ref, g, offsets, 0).max() > 2 * gr.BIN_CHUNK
        if name == "A-hash":
            # COMBINE = 2 (level 2, dense: corner 0's row names the cell): runs of live samples in one cell, cut at rows of 16 lanes
            key = np.where(live[2], ref.rows[2, 0], -1)
            start, length = _runs(key, 16)
            inside = (length >= 2) & (start % 16 > 0) & ((start + length - 1) % 16 < 15)
            assert inside.sum() >= 20, inside.sum()
            i = np.arange(1, ref.B)
            crossing = (key[1:] == key[:-1]) & (key[1:] >= 0) & (i % 16 == 0)
            assert crossing.sum() >= 20 and (crossing & (i % 64 == 0)).any() and (crossing & (i % 1024 == 0)).any()
            assert (length == 16).any()                                             # a run that fills its row (all four steps of the scan add)
            assert ((length == 13) & (start % 16 == 2)).any()                       # ... and one of 13 strictly inside
            for k in (2, 3, 4, 5, 6, 7):
                assert (length == k).any(), k
            # a dead sample inside a cell's run ends it: live, dead, live in one cell
            cell = np.where(ref.inr, ref.rows[2, 0], -1)
            mid = (cell[2:] == cell[1:-1]) & (cell[:-2] == cell[1:-1]) & (cell[1:-1] >= 0) & live[2, 2:] & live[2, :-2] & ~live[2, 1:-1]
            assert mid.sum() >= 5, mid.sum()
            # COMBINE = 1 (levels 0 and 1 with coarse_image = 0): runs of equal rows per corner, cut at waves
            longest = 0
            for l in (0, 1):
                for corner in (0, 7):
                    key = np.where(live[l], ref.rows[l, corner], -1)
                    start, length = _runs(key, 64)
                    longest = max(longest, int(length.max()))
                    assert ((length >= 2) & (start % 64 > 0) & ((start + length - 1) % 64 < 63)).sum() >= 20
                    assert ((key[1:] == key[:-1]) & (key[1:] >= 0) & (i % 64 == 0)).any()
            assert longest >= 17                                               # longer than a row of 16: the wave scan's later steps
            # the gradient's zeros: dead tails, dead pairs among the live, one-channel samples, -0.0
            g3 = g.reshape(ref.B, L, 2)
            assert (~live[:, :4995] & ref.inr[None, :4995]).mean() > 0.3 and live.mean() > 0.3
            assert ((g3[:, :, 0] == 0) & (g3[:, :, 1] != 0)).sum() > 1000
            assert (np.signbit(g3) & (g3 == 0)).sum() >= 40
            assert not ref.inr[[100, 200, 500, 600]].any() and ref.inr[[400, 401]].all()
    print("fp32 oracle, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst_oracle.items()))


if __name__ == "__main__":
    sys.exit(_small_table_then_a_larger_one())
