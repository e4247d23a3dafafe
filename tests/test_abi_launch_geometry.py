"""pnr_launch_geometry on the host (no GPU needed): the workgroups a capped-grid entry launches for a batch and the rows a workgroup handles per
trip of its tile loop, as the launcher's own helper computes them.  tests/test_gpu_grid_caps.py takes its batches from this query, so that a
retuned cap moves the tests with it.  An additive entry: the ABI version stays 10."""
import ctypes
import os
import re

import pytest

from palettenerf_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("pnr_palette_heads_forward", "pnr_palette_heads_backward", "pnr_palette_smooth_forward", "pnr_palette_smooth_backward",
         "pnr_palette_smooth_points", "pnr_palette_train_shade_forward", "pnr_palette_train_shade_backward", "pnr_nerf_field_forward",
         "pnr_nerf_density_forward", "pnr_mlp_forward", "pnr_mlp_backward")
INVALID = -1
FAR = 1 << 31      # a batch beyond every cap (and inside every entry's 32-bit row count)


def query(name, rows):
    wg, rpt = ctypes.c_uint32(0xDEAD), ctypes.c_uint32(0xDEAD)
    rc = _lib.load().pnr_launch_geometry(name.encode(), rows, ctypes.byref(wg), ctypes.byref(rpt))
    return rc, wg.value, rpt.value


def test_the_entry_is_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    assert re.search(r"\bint pnr_launch_geometry\s*\(\s*const char\* entry, uint64_t rows, uint32_t\* workgroups, uint32_t\* rows_per_trip\)", hdr)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert _lib.SIGNATURES["pnr_launch_geometry"] == [ctypes.c_char_p, ctypes.c_uint64, u32p, u32p]
    assert hasattr(_lib.load(), "pnr_launch_geometry") and _lib.load().pnr_abi_version() == 10


@pytest.mark.parametrize("name", NAMES)
def test_every_listed_name_answers(name):
    rc, wg, rpt = query(name, 1000)
    assert rc == 0 and wg >= 1 and rpt >= 1 and wg * rpt >= 1000        # below every cap: one trip covers the batch
    assert _lib.launch_geometry(name, 1000) == (wg, rpt)
    assert _lib.SIGNATURES[name]                                          # the names are entries of the library, spelled as it exports them


@pytest.mark.parametrize("name", NAMES)
def test_workgroups_grow_with_the_batch_up_to_a_constant(name):
    rc, cap, rpt = query(name, FAR)
    assert rc == 0 and 0 < cap * rpt < FAR
    K = cap * rpt
    rows = sorted({1, 2, rpt - 1, rpt, rpt + 1, 3 * rpt, 1000, 9010, 50077, 70001, K // 2, K - rpt, K - rpt + 1, K - 1, K, K + 1, K + rpt, 2 * K,
                   3 * K + 7, 1 << 24, 1 << 30, FAR})
    got = []
    for r in rows:
        rc, wg, rpt_r = query(name, r)
        assert rc == 0 and rpt_r == rpt, r                                # the tile does not depend on the batch
        assert wg == min(-(-r // rpt), cap), (r, wg)                      # one workgroup per tile until the cap
        got.append(wg)
    assert got == sorted(got) and got[-1] == cap and got[rows.index(K)] == cap


@pytest.mark.parametrize("name", NAMES)
def test_the_second_trip_starts_one_row_past_cap_times_tile(name):
    _, cap, rpt = query(name, FAR)
    K = cap * rpt
    for rows, second in ((K - 1, False), (K, False), (K + 1, True), (K + 2 * rpt + 3, True)):
        rc, wg, rpt_r = query(name, rows)
        assert rc == 0 and (rows > wg * rpt_r) == second, rows


def test_names_without_a_capped_grid_and_missing_pointers_are_invalid():
    lib = _lib.load()
    wg, rpt = ctypes.c_uint32(7), ctypes.c_uint32(7)
    for name in (b"", b"pnr_no_such_entry", b"pnr_palette_field_forward", b"pnr_march_rays", b"pnr_launch_geometry", b"PNR_MLP_FORWARD",
                 b"pnr_mlp_forward ", b"pnr_mlp_forwar"):
        assert lib.pnr_launch_geometry(name, 1000, ctypes.byref(wg), ctypes.byref(rpt)) == INVALID, name
        assert (wg.value, rpt.value) == (7, 7)                            # nothing is written for a refused name
    assert lib.pnr_launch_geometry(None, 1000, ctypes.byref(wg), ctypes.byref(rpt)) == INVALID
    assert lib.pnr_launch_geometry(b"pnr_mlp_forward", 1000, None, ctypes.byref(rpt)) == INVALID
    assert lib.pnr_launch_geometry(b"pnr_mlp_forward", 1000, ctypes.byref(wg), None) == INVALID
    # more rows than the entry's own uint32 row count can express; pnr_palette_smooth_points counts up to three elements per row
    assert query("pnr_palette_heads_forward", 1 << 32)[0] == INVALID and query("pnr_mlp_backward", 1 << 40)[0] == INVALID
    assert query("pnr_palette_smooth_points", 1 << 32)[0] == 0 and query("pnr_palette_smooth_points", 3 << 32)[0] == INVALID


def test_the_forward_and_backward_caps_that_differ_are_reported_apart():
    """The shade and MLP backward launch fewer workgroups than their forward (one partial row of the reduced gradient per workgroup)."""
    for fwd, bwd in (("pnr_palette_train_shade_forward", "pnr_palette_train_shade_backward"), ("pnr_mlp_forward", "pnr_mlp_backward")):
        (_, cf, rf), (_, cb, rb) = query(fwd, FAR), query(bwd, FAR)
        assert rf == rb and cb < cf and cf % cb == 0                      # one batch past the larger cap is past both, on coinciding tiles


def mlp_desc(dims):
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def test_the_partial_row_buffers_are_sized_by_the_reported_workgroups():
    lib = _lib.load()
    _, shade_cap, _ = query("pnr_palette_train_shade_backward", FAR)
    for nb in (1, 4, 16):
        assert lib.pnr_palette_train_shade_workspace_bytes(nb) == shade_cap * nb * 3 * 4      # sized for the cap whatever the batch
    for rows in (1, 255, 256, 257, 20016, 131072, 131073, FAR):
        assert query("pnr_palette_train_shade_backward", rows)[1] <= shade_cap
    for dims in ((31, 64, 64, 3), (32, 64, 16), (7, 20, 40)):
        d = mlp_desc(dims)
        dw_floats = sum(a * b for a, b in zip(dims, dims[1:]))
        for rows in (1, 127, 128, 129, 4097, 32768, 32769, 50077, 627000, FAR):
            wg = query("pnr_mlp_backward", rows)[1]
            assert lib.pnr_mlp_backward_workspace_bytes(ctypes.byref(d), rows) == wg * dw_floats * 4, (dims, rows)
