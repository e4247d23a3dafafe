"""The palette extraction's entries (include/pnr.h, "palette extraction, front end") are declared, bound and exported, the ABI version is
unchanged, and every refusal returns its code before a launch.  No GPU: the pointers are dummies that nothing may follow."""
import ctypes
import os
import re

from palettenerf_amd import _lib

INVALID, UNSUPPORTED, OK = -1, -2, 0
P = 64      # a non-null, 16-byte aligned address that is never read
ENTRIES = ("pnr_extract_accumulate", "pnr_extract_kmeans_workspace_bytes", "pnr_extract_kmeans")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnr.h")


def accumulate_args(**over):
    a = _lib.ExtractAccumulateArgs()
    a.H, a.W, a.channels, a.image_format, a.thresh = 4, 5, 3, _lib.IMAGE_FP32, 0.5
    a.weights_sum = a.pixels = a.counts_coarse = a.counts_fine = a.total = P
    for k, v in over.items():
        setattr(a, k, v)
    return a


def kmeans_args(**over):
    a = _lib.ExtractKmeansArgs()
    a.counts_coarse = a.counts_fine = a.total = a.workspace = a.centers = a.center_weights = a.info = P
    a.tau, a.tol, a.max_iter = 8e-3, 1e-4, 300
    a.workspace_bytes = _lib.load().pnr_extract_kmeans_workspace_bytes()
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entries_are_declared_bound_and_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    header = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.pnr_extract_kmeans_workspace_bytes() == 32768 * 8
    for macro, value in (("PNR_EXTRACT_COARSE_BINS", _lib.EXTRACT_COARSE_BINS), ("PNR_EXTRACT_FINE_BINS", _lib.EXTRACT_FINE_BINS),
                         ("PNR_EXTRACT_MAX_K", _lib.EXTRACT_MAX_K), ("PNR_EXTRACT_EMPTIED", _lib.EXTRACT_EMPTIED),
                         ("PNR_EXTRACT_NO_CENTER", _lib.EXTRACT_NO_CENTER), ("PNR_EXTRACT_TOO_MANY", _lib.EXTRACT_TOO_MANY),
                         ("PNR_EXTRACT_FEW_POINTS", _lib.EXTRACT_FEW_POINTS)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    for i, rule in enumerate(("CAP", "LABELS", "SHIFT")):
        assert re.search(r"#define PNR_EXTRACT_STOP_%s %d\b" % (rule, i), header)
    assert _lib.EXTRACT_STOP == ("max_iter", "labels", "shift")


def test_struct_mirrors_have_the_header_fields_in_order():
    header = open(HEADER).read()
    for struct, mirror in (("pnr_extract_accumulate_args", _lib.ExtractAccumulateArgs), ("pnr_extract_kmeans_args", _lib.ExtractKmeansArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"[\s\*]", "", n).split(" ")[-1] for n in re.sub(r"^(const\s+)?\w+[\s\*]+", "", decl).split(",")]
        assert names == [f[0] for f in mirror._fields_], struct


def test_accumulate_refuses_before_a_launch():
    fn = _lib.load().pnr_extract_accumulate
    assert fn(None, None) == INVALID
    for fmt in (-1, 3, 7):
        assert fn(ctypes.byref(accumulate_args(image_format=fmt)), None) == UNSUPPORTED, fmt
    for ch in (0, 1, 2, 5):
        assert fn(ctypes.byref(accumulate_args(channels=ch)), None) == UNSUPPORTED, ch
    for name in ("weights_sum", "pixels", "counts_coarse", "counts_fine", "total"):
        assert fn(ctypes.byref(accumulate_args(**{name: None})), None) == INVALID, name
    # N = 0: PNR_OK, nothing touched (not even looked at: the pointers may be NULL)
    for hw in ((0, 5), (4, 0), (0, 0)):
        assert fn(ctypes.byref(accumulate_args(H=hw[0], W=hw[1], weights_sum=None, pixels=None, counts_fine=None)), None) == OK, hw
    # a row stride below the row, or not a multiple of the element; a base not aligned to the element
    assert fn(ctypes.byref(accumulate_args(row_stride_bytes=5 * 3 * 4 - 4)), None) == INVALID
    assert fn(ctypes.byref(accumulate_args(row_stride_bytes=5 * 3 * 4 + 2)), None) == INVALID
    assert fn(ctypes.byref(accumulate_args(pixels=P + 2)), None) == INVALID
    assert fn(ctypes.byref(accumulate_args(image_format=_lib.IMAGE_FP16, pixels=P + 1)), None) == INVALID
    # an unknown format wins over a NULL pointer and over N = 0: the order of the checks in the header
    assert fn(ctypes.byref(accumulate_args(image_format=9, pixels=None, H=0)), None) == UNSUPPORTED


def test_kmeans_refuses_before_a_launch():
    fn = _lib.load().pnr_extract_kmeans
    assert fn(None, None) == INVALID
    for name in ("counts_coarse", "counts_fine", "total", "workspace", "centers", "center_weights", "info"):
        assert fn(ctypes.byref(kmeans_args(**{name: None})), None) == INVALID, name
    assert fn(ctypes.byref(kmeans_args(workspace_bytes=32768 * 8 - 1)), None) == INVALID
    assert fn(ctypes.byref(kmeans_args(workspace=P + 4)), None) == INVALID
    assert fn(ctypes.byref(kmeans_args(max_iter=0)), None) == INVALID
    assert fn(ctypes.byref(kmeans_args(tau=-1.0)), None) == INVALID
    assert fn(ctypes.byref(kmeans_args(tol=float("nan"))), None) == INVALID


def test_launch_geometry_answers_for_the_accumulate_entry():
    assert _lib.launch_geometry("pnr_extract_accumulate", 1) == (1, 1024)
    assert _lib.launch_geometry("pnr_extract_accumulate", 1025) == (2, 1024)
    assert _lib.launch_geometry("pnr_extract_accumulate", 800 * 800) == (256, 1024)
