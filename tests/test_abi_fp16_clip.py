"""ABI 8: pnr_interleave_tables3_half (the half triple of the -O clip-head frame) is declared, bound and validates its arguments (no compute calls)."""
import ctypes


def test_abi_version_and_half_triple_entry_point():
    from palettenerf_amd import _lib
    lib = _lib.load()
    assert lib.pnr_abi_version() >= 8
    assert "pnr_interleave_tables3_half" in _lib.SIGNATURES
    fn = lib.pnr_interleave_tables3_half
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert fn(None, None, None, ctypes.c_uint64(0), None, None) == 0            # nothing to do
    assert fn(p, p, None, ctypes.c_uint64(4), p, None) == -1                    # a missing table: invalid, nothing launched
    assert fn(p, p, p, ctypes.c_uint64(4), None, None) == -1                    # no output
