"""profiles/kernel_coverage.py on a machine without a GPU: the inventory of compiled gfx950 kernels read from the per-unit objects of the product build,
and the one spelling both the inventory and the profiler's traces are brought to.  A missing LLVM tool fails here as a missing hipcc fails the build."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cov():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "profiles", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def names(cov):
    inv = cov.inventory()       # (of the objects __graft_entry__.build() left; a tree that was never built has none and fails here)
    return inv, {k for ks in inv.values() for k in ks}


def test_inventory_lists_the_compiled_kernels(names):
    inv, flat = names
    assert flat and all(inv.values())
    assert all(k.startswith("pnr::") for k in flat), sorted(k for k in flat if not k.startswith("pnr::"))
    assert "options" not in inv and "launch_geometry" not in inv       # units without device code are skipped, not listed empty
    assert {"frame", "linear", "shencoder", "gridencoder", "mlp", "raymarch"} <= set(inv)
    march = {f"pnr::k_frame_march<{mip}, {pow2}, 1>" for mip in ("true", "false") for pow2 in ("true", "false")} | {"pnr::k_frame_march<true, true, 2>"}
    assert march <= set(inv["frame"]) and sum("k_frame_march<" in k for k in flat) == 5
    wgrad = {f"pnr::k_linear_wgrad<{x}, {dy}, {a}, {b}>" for x in ("float", "__half") for dy in ("float", "__half") for a in (1, 2) for b in (1, 2)}
    assert len(wgrad) == 16 and wgrad <= set(inv["linear"]) and sum("k_linear_wgrad<" in k for k in flat) == 16
    assert {f"pnr::k_sh_cat_fwd<{d}>" for d in range(1, 8)} <= set(inv["shencoder"])


@pytest.mark.parametrize("raw,want", [
    # rocprofv3's Kernel_Name column: demangled, with the return type of a template and the parameter list; older versions keep the `.kd`
    ("void pnr::k_frame_march<true, false, 1>(pnr::FrameCtl const*, pnr::FrameCtl*, int const*, int*, pnr::MarchArgs, unsigned int)", "pnr::k_frame_march<true, false, 1>"),
    ("void pnr::k_frame_march<true, true, 2>(pnr::FrameCtl const*, pnr::FrameCtl*) [clone .kd]", "pnr::k_frame_march<true, true, 2>"),
    ("void pnr::k_linear_wgrad<__half, float, 2, 1>(__half const*, float const*, float*, unsigned int, unsigned int, unsigned int).kd", "pnr::k_linear_wgrad<__half, float, 2, 1>"),
    ('"void pnr::k_sh_cat_fwd<6>(float const*, float const*, float*, unsigned int, unsigned int)"', "pnr::k_sh_cat_fwd<6>"),
    # readelf's symbol after c++filt: no `void` in front of a plain function, `.kd` behind the parameter list
    ("pnr::k_sigma_geo_cat_bwd(float const*, float*, unsigned int, unsigned int).kd", "pnr::k_sigma_geo_cat_bwd"),
    ("pnr::k_occ_lookup(pnr::OccArgs)", "pnr::k_occ_lookup"),
    ("void pnr::k_frame_unsort_outputs<32u>(float const*, float*, int const*, unsigned int).kd", "pnr::k_frame_unsort_outputs<32u>"),
    # parentheses inside template brackets are not the parameter list
    ("void pnr::k_example<(pnr::Kind)1, true>(pnr::Args<(pnr::Kind)1>)", "pnr::k_example<(pnr::Kind)1, true>"),
])
def test_normaliser_brings_both_spellings_to_the_inventory_name(cov, names, raw, want):
    assert cov.normalise(raw) == want
    if "k_example" not in want:
        assert want in names[1]


def test_launched_reads_every_trace_file_and_only_pnr_names(cov, tmp_path):
    (tmp_path / "host" / "child").mkdir(parents=True)
    head = '"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"\n'
    row = '"KERNEL_DISPATCH",1,1,7,"{}",1,10,20\n'
    (tmp_path / "host" / "11_kernel_trace.csv").write_text(head + row.format("void pnr::k_sh_cat_fwd<2>(float const*, float*)") * 2
                                                           + row.format("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>(int, float)"))
    (tmp_path / "host" / "child" / "12_kernel_trace.csv").write_text(head + row.format("pnr::k_occ_lookup(pnr::OccArgs).kd") + row.format("void pnr::k_sh_cat_fwd<2>(float const*, float*)"))
    assert cov.launched(str(tmp_path)) == {"pnr::k_sh_cat_fwd<2>": 3, "pnr::k_occ_lookup": 1}
