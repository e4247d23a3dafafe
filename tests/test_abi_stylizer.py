"""The Stylizer fit on the host: pnr_stylizer_fit (palette/gui.py:153-194) is declared, bound and exported and validates before any launch
(no GPU needed).  An additive entry: the ABI version stays 10."""
import ctypes
import os
import re

from palettenerf_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "pnr_stylizer_fit"
INVALID, UNSUPPORTED = -1, -2
P = 256     # any non-null address: nothing below reaches a launch
REQUIRED = ("radiance", "omega", "offsets", "palette", "target", "dI", "dP", "ddelta", "lr")
MOMENTUM = ("mom_dI", "mom_dP", "mom_ddelta")


def args(M=8, nb=4, iters=10, **over):
    a = _lib.StylizerFitArgs(M=M, num_basis=nb, iters=iters, momentum=0.9, lambda_arap=0.1)
    for k in REQUIRED:
        setattr(a, k, P)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def fit(a):
    return _lib.load().pnr_stylizer_fit(ctypes.byref(a), None)


def test_the_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint " + NAME + r"\s*\(\s*const pnr_stylizer_fit_args\s*\*", bare)
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert _lib.SIGNATURES[NAME] == [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.pnr_abi_version() == 10
    assert re.search(r"#define PNR_STYLIZER_MAX_POINTS\s+%d\b" % _lib.STYLIZER_MAX_POINTS, hdr) and _lib.STYLIZER_MAX_POINTS >= 512
    assert re.search(r"#define PNR_STYLIZER_MAX_ITERS\s+%d\b" % _lib.STYLIZER_MAX_ITERS, hdr) and _lib.STYLIZER_MAX_ITERS == 10000


def test_the_struct_mirrors_the_header_field_for_field():
    bare = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    body = re.search(r"typedef struct pnr_stylizer_fit_args \{(.*?)\} pnr_stylizer_fit_args;", bare, flags=re.S).group(1)
    names, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.rsplit("*", 1) if "*" in decl else decl.split(None, 1)
        for n in rest.split(","):
            names.append(n.strip())
            kinds.append("ptr" if "*" in decl else ctype.strip())
    assert names == [f[0] for f in _lib.StylizerFitArgs._fields_]
    want = {"ptr": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float}
    assert [want[k] for k in kinds] == [f[1] for f in _lib.StylizerFitArgs._fields_]


def test_the_header_cites_the_reference_block():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    at = hdr.index("int " + NAME)
    block = hdr[hdr.rindex("/* ----", 0, at):at]
    assert "palette/gui.py:153-194" in block and "palette/renderer.py:150-183" in block


def test_limits_are_unsupported_before_any_launch():
    for over in (dict(nb=3), dict(nb=_lib.MAX_BASIS + 1), dict(M=_lib.STYLIZER_MAX_POINTS + 1), dict(iters=_lib.STYLIZER_MAX_ITERS + 1)):
        assert fit(args(**over)) == UNSUPPORTED, over
        a = args(**over)
        for k in REQUIRED:
            setattr(a, k, None)
        assert fit(a) == UNSUPPORTED, over          # the shape is checked first, as in the smooth and shade entries
    assert fit(args(nb=3, M=0)) == UNSUPPORTED and fit(args(iters=0, M=_lib.STYLIZER_MAX_POINTS + 1)) == UNSUPPORTED


def test_an_empty_fit_is_ok_and_touches_nothing():
    for over in (dict(M=0), dict(iters=0), dict(M=0, iters=0)):
        for nb in (4, _lib.MAX_BASIS):
            a = args(nb=nb, **over)
            assert fit(a) == 0, (over, nb)
            for k in REQUIRED:
                setattr(a, k, None)
            assert fit(a) == 0, (over, nb)           # nothing is read


def test_every_required_pointer_is_checked():
    assert _lib.load().pnr_stylizer_fit(None, None) == INVALID
    for k in REQUIRED:
        assert fit(args(**{k: None})) == INVALID, k
    for k in MOMENTUM:                                # all three buffers or none
        assert fit(args(**{k: P})) == INVALID, k
        assert fit(args(**{m: P for m in MOMENTUM if m != k})) == INVALID, k
    assert fit(args(has_momentum=1)) == INVALID      # a run cannot continue from buffers it was not given
