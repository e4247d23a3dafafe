"""Guard bands around every array of the C-ABI entries of the training step and the frame loop (tests/guarded.py): no byte written outside an
output or a workspace, no result that depends on a byte outside an input.

Every case calls its entry twice through the C ABI: on plain tensors, and with every device input inside NaN (or meaning-preserving integer)
surroundings, every output inside sentinel bytes and the workspace at exactly the size its *_workspace_bytes function returns -- once with every
array on a 256-byte boundary, once at the weakest alignment the entry's comment in include/pnr.h allows.  It asserts (a) every guard byte is
untouched, (b) every guarded output equals the plain call's bit for bit, (c) no output holds a NaN the plain call did not produce.  The plain
call's values are what the other test files hold to their references; this file needs none of its own.

Compared under a bound instead of bit for bit (float atomics: two calls need not agree), the plain and the guarded call each against the float64 gradient:
grad_embeddings of pnr_grid_encode_backward and of pnr_grid_encode_backward_binned under tests/grid_reference.py's table_grad_bound, grad_table of
pnr_background_backward under tests/test_gpu_background_train.py's BOUND; rows that no sample reaches must stay exactly zero.

ENTRIES (readable without a GPU) maps every entry name to the cases that call it; tests/test_guard_bands_host.py checks it against the header."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib
from palettenerf_amd._torch_glue import stream_ptr
from tests import guarded
from tests import grid_reference as gr

ENTRIES = {}      # entry name -> [test function names]
ERR_INVALID, ERR_UNSUPPORTED, ERR_ALIGNMENT = -1, -2, -4
u64 = ctypes.c_uint64


def guards(*entries):
    """Marks a GPU case and registers the entries it calls."""
    def deco(fn):
        for e in entries:
            ENTRIES.setdefault(e, []).append(fn.__name__)
        return pytest.mark.gpu(fn)
    return deco


def abi(name, *args):
    """The entry's return code (the wrappers of palettenerf_amd raise on a refusal; the refusal cases want the code)."""
    return getattr(_lib.load(), name)(*args, stream_ptr())


def nbytes_of(name, *args):
    return int(getattr(_lib.load(), name)(*args))


class Arr:
    def __init__(self, role, t=None, around=None, weak=None, nbytes=None, zero=False):
        self.role, self.t, self.around, self.nbytes, self.zero = role, t, around, nbytes, zero
        self.weak = weak if weak is not None else (256 if role == "ws" else t.element_size())


def I(t, around=None, weak=None):
    """A device input: NaN bytes around a floating array, `around` (values valid for the array's meaning, or a byte for plain data) around an integer one."""
    return Arr("in", t, around, weak)


def O(t, weak=None):
    """A device output (or an array updated in place), pre-filled with `t` as the entry's caller in palettenerf_amd pre-fills it."""
    return Arr("out", t, None, weak)


def IO(t, around, weak=None):
    """An index array the entry updates in place: surrounded like an input (values valid for its meaning), compared like an output."""
    return Arr("io", t, around, weak)


def WS(nbytes, weak=256, zero=False):
    """The workspace: exactly `nbytes` bytes.  weak: the alignment include/pnr.h documents (256 where it documents none: the allocator's)."""
    return Arr("ws", None, None, weak, int(nbytes), zero)


EMPTY = 0.25      # what an output the wrappers allocate with torch.empty holds before the call, here


def empty(*shape, dtype=torch.float32, device="cuda"):
    return torch.full(shape, EMPTY, dtype=dtype, device=device)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def nans(t):
    return int(torch.isnan(t).sum()) if t.dtype.is_floating_point else 0


def plain_tensors(arrays):
    a = {}
    for k, v in arrays.items():
        if v is None:
            a[k] = None
        elif v.role == "ws":
            a[k] = (torch.zeros if v.zero else torch.empty)(max(v.nbytes, 16), dtype=torch.uint8, device="cuda")
        else:
            a[k] = v.t.clone()
    return a


def guarded_tensors(arrays, mode):
    bufs, views = {}, {}
    for k, v in arrays.items():
        if v is None:
            views[k] = None
            continue
        align = 0 if mode == "aligned" else (mode if isinstance(mode, int) else v.weak)
        if v.role == "ws":
            bufs[k], views[k] = guarded.workspace(v.nbytes, "cuda", align)
            if v.zero:
                views[k].zero_()
        elif v.role in ("in", "io"):
            bufs[k], views[k] = guarded.inp(v.t, align, v.around)
        else:
            bufs[k], views[k] = guarded.out(v.t.shape, v.t.dtype, v.t.device, align)
            views[k].copy_(v.t)
    return bufs, views


def check(call, arrays, what="", expect=0, modes=("aligned", "weak"), close=None, plain=True):
    """call(a) -> return code, a = {name: tensor or None}.  expect == 0: the plain call, then the guarded call per alignment mode, with (a), (b), (c);
    close = {output name: fn(got, plain tensor)} for the outputs float atomics make irreproducible.  expect != 0: the guarded call is refused with
    that code and not one byte of its outputs (or guards) changes.  -> (plain tensors, [guarded tensors per mode])."""
    ref = None
    if expect == 0 and plain:
        ref = plain_tensors(arrays)
        rc = call(ref)
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: the plain call returned {rc}"
    results = []
    for mode in modes:
        bufs, a = guarded_tensors(arrays, mode)
        rc = call(a)
        torch.cuda.synchronize()
        assert rc == expect, f"{what} [{mode}]: returned {rc}, expected {expect}"
        for k, v in arrays.items():
            if v is None:
                continue
            assert guarded.untouched(bufs[k], a[k]), f"{what} [{mode}] {k} ({v.role}): {guarded.last_report}"
            if v.role == "in":
                assert same_bits(a[k], v.t), f"{what} [{mode}]: input {k} was written"
            elif v.role in ("out", "io") and expect != 0:
                assert same_bits(a[k], v.t), f"{what} [{mode}]: refused, yet output {k} changed"
            elif v.role in ("out", "io") and ref is not None:
                if close and k in close:
                    close[k](a[k], ref[k])
                    continue
                if not same_bits(a[k], ref[k]):
                    diff = torch.nonzero((a[k] != ref[k]).view(-1))
                    first = int(diff[0]) if diff.numel() else -1
                    raise AssertionError(f"{what} [{mode}]: output {k} differs from the plain call's in {diff.numel()} of {a[k].numel()} elements, "
                                         f"first at flat index {first}; NaNs {nans(a[k])} against {nans(ref[k])}")
                assert nans(a[k]) == nans(ref[k])
        results.append(a)
    return ref, results


def p(t):
    return None if t is None else t.data_ptr()


def rnd(seed, *shape, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def uni(seed, *shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).float().cuda()


class option:
    """pnr_set_option for the length of a with block (back to `default` behind it)."""

    def __init__(self, name, value, default):
        self.name, self.value, self.default = name.encode(), value, default

    def __enter__(self):
        assert _lib.load().pnr_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        _lib.load().pnr_set_option(self.name, self.default)


# ================================================================ optimiser step: pnr_adam_step, _amp, pnr_grad_check, pnr_ema_update, _swap
# k_adam / k_grad_check / k_ema walk 2048-element chunks (csrc/adam.hip); a whole chunk takes the eight-loads-in-flight path
ADAM_TABLES = {"ends": (1, 2047, 2048, 2049), "three": (2049, 2047, 2048), "single-1": (1,), "mixed-0": (2048, 0, 1, 2049, 0, 2047)}


def adam_arrays(ns, seed):
    arrays = {}
    for k, n in enumerate(ns):
        arrays[f"p{k}"] = O(rnd(seed + 4 * k, n))
        arrays[f"g{k}"] = I(rnd(seed + 4 * k + 1, n, scale=0.1))
        arrays[f"m{k}"] = O(rnd(seed + 4 * k + 2, n, scale=0.1))
        arrays[f"v{k}"] = O(rnd(seed + 4 * k + 3, n, scale=0.1).square())
    return arrays


def adam_table(a, ns):
    arr = (_lib.AdamTensor * len(ns))()
    for k, n in enumerate(ns):
        arr[k].param, arr[k].grad, arr[k].exp_avg, arr[k].exp_avg_sq, arr[k].n = p(a[f"p{k}"]), p(a[f"g{k}"]), p(a[f"m{k}"]), p(a[f"v{k}"]), n
    return arr


def adam_scalars(step=3, lr=1e-2, b1=0.9, b2=0.99, eps=1e-15):
    sc = _lib.AdamScalars()
    sc.one_minus_beta1, sc.beta2, sc.one_minus_beta2 = 1 - b1, b2, 1 - b2
    sc.bias_correction2_sqrt, sc.eps, sc.neg_step_size, sc.inv_grad_scale = (1 - b2 ** step) ** 0.5, eps, -(lr / (1 - b1 ** step)), 1.0
    return sc


@guards("pnr_adam_step")
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_adam_step(cuda, table):
    ns = ADAM_TABLES[table]
    arrays, sc = adam_arrays(ns, 100), adam_scalars()
    check(lambda a: abi("pnr_adam_step", adam_table(a, ns), len(ns), ctypes.byref(sc)), arrays, f"pnr_adam_step {ns}")


@guards("pnr_grad_check")
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_grad_check_reads_nothing_outside_the_gradients(cuda, table):
    ns = ADAM_TABLES[table]
    arrays = {k: v for k, v in adam_arrays(ns, 200).items() if k[0] == "g"}
    arrays["found_inf"] = O(torch.zeros(1, device="cuda"))

    def call(a):
        arr = (_lib.AdamTensor * len(ns))()
        for k, n in enumerate(ns):
            arr[k].grad, arr[k].n = p(a[f"g{k}"]), n
        return abi("pnr_grad_check", arr, len(ns), p(a["found_inf"]))

    _, res = check(call, arrays, f"pnr_grad_check {ns}")        # the gradients sit in NaN surroundings: a read outside them raises the flag
    for a in res:
        assert float(a["found_inf"]) == 0.0
    last = max(k for k, n in enumerate(ns) if n > 0)
    arrays[f"g{last}"].t[-1] = float("inf")                     # one real inf, the last element of the last tensor
    _, res = check(call, arrays, f"pnr_grad_check {ns} inf")
    for a in res:
        assert float(a["found_inf"]) == 1.0


@guards("pnr_adam_step_amp")
@pytest.mark.parametrize("found", [0.0, 1.0])
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_adam_step_amp(cuda, table, found):
    ns = ADAM_TABLES[table]
    arrays = adam_arrays(ns, 300)
    arrays["scale"] = I(torch.full((1,), 1024.0, device="cuda"))
    arrays["found_inf"] = I(torch.full((1,), found, device="cuda"))
    arrays["state"] = O(torch.zeros(3, dtype=torch.int32, device="cuda"))
    rows = (_lib.AdamScalars * 8)()
    for r in range(3):
        rows[r] = adam_scalars(step=5 - r)

    def call(a):
        ctl = _lib.AdamAmpCtl()
        ctl.scale, ctl.found_inf, ctl.state, ctl.skipped_base, ctl.parity = p(a["scale"]), p(a["found_inf"]), p(a["state"]), 0, 0
        return abi("pnr_adam_step_amp", adam_table(a, ns), len(ns), rows, 3, ctypes.byref(ctl))

    _, res = check(call, arrays, f"pnr_adam_step_amp {ns} found_inf={found}")
    for a in res:
        assert a["state"].tolist() == [0, int(found), 0]


def ema_arrays(ns, seed):
    arrays = {}
    for k, n in enumerate(ns):
        arrays[f"p{k}"] = rnd(seed + 2 * k, n)
        arrays[f"s{k}"] = rnd(seed + 2 * k + 1, n)
    return arrays


def ema_table(a, ns):
    arr = (_lib.EmaTensor * len(ns))()
    for k, n in enumerate(ns):
        arr[k].param, arr[k].shadow, arr[k].n = p(a[f"p{k}"]), p(a[f"s{k}"]), n
    return arr


@guards("pnr_ema_update")
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_ema_update(cuda, table):
    ns = ADAM_TABLES[table]
    t = ema_arrays(ns, 400)
    arrays = {k: (I(v) if k[0] == "p" else O(v)) for k, v in t.items()}
    w = ctypes.c_float(1.0 - 0.95)
    ref, _ = check(lambda a: abi("pnr_ema_update", ema_table(a, ns), len(ns), w), arrays, f"pnr_ema_update {ns}")
    for k, n in enumerate(ns):      # torch_ema's three elementwise kernels, rounding for rounding
        tmp = (t[f"s{k}"] - t[f"p{k}"]) * w.value
        assert torch.equal(ref[f"s{k}"], t[f"s{k}"] - tmp), (table, k)


@guards("pnr_ema_swap")
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_ema_swap(cuda, table):
    ns = ADAM_TABLES[table]
    t = ema_arrays(ns, 500)
    ref, _ = check(lambda a: abi("pnr_ema_swap", ema_table(a, ns), len(ns)), {k: O(v) for k, v in t.items()}, f"pnr_ema_swap {ns}")
    for k, n in enumerate(ns):
        assert torch.equal(ref[f"p{k}"], t[f"s{k}"]) and torch.equal(ref[f"s{k}"], t[f"p{k}"])


# ================================================================ SH encoder and the sigma / geo_feat seam (256 rows per workgroup)
SH_ROWS = (1, 255, 256, 257)


def unit_dirs(seed, B):
    d = rnd(seed, B, 3)
    return d / d.norm(dim=1, keepdim=True)


@guards("pnr_sh_encode_forward", "pnr_sh_encode_backward")
@pytest.mark.parametrize("degree", [1, 4, 7, 8])
@pytest.mark.parametrize("B", SH_ROWS)
def test_sh_encode(cuda, B, degree):
    dirs, n = unit_dirs(B + degree, B), degree * degree
    for with_dy in (False, True):
        arrays = dict(inputs=I(dirs), outputs=O(empty(B, n)), dy_dx=O(empty(B, 3 * n)) if with_dy else None)
        ref, _ = check(lambda a: abi("pnr_sh_encode_forward", p(a["inputs"]), p(a["outputs"]), B, 3, degree, p(a["dy_dx"])), arrays,
                       f"pnr_sh_encode_forward B={B} degree={degree} dy_dx={with_dy}")
    arrays = dict(grad=I(rnd(7, B, n)), inputs=I(dirs), dy_dx=I(ref["dy_dx"]), grad_inputs=O(torch.zeros(B, 3, device="cuda")))
    check(lambda a: abi("pnr_sh_encode_backward", p(a["grad"]), p(a["inputs"]), B, 3, degree, p(a["dy_dx"]), p(a["grad_inputs"])), arrays,
          f"pnr_sh_encode_backward B={B} degree={degree}")


@guards("pnr_sh_encode_cat_forward")
@pytest.mark.parametrize("degree,tail", [(1, 1), (1, 15), (1, 60), (4, 1), (4, 15), (7, 1), (7, 15)])
@pytest.mark.parametrize("B", SH_ROWS)
def test_sh_encode_cat(cuda, B, degree, tail):
    arrays = dict(inputs=I(unit_dirs(B, B)), tail=I(rnd(tail, B, tail)), outputs=O(empty(B, degree * degree + tail)))
    check(lambda a: abi("pnr_sh_encode_cat_forward", p(a["inputs"]), p(a["tail"]), tail, p(a["outputs"]), B, degree), arrays,
          f"pnr_sh_encode_cat_forward B={B} degree={degree} tail={tail}")


@guards("pnr_sigma_geo_cat_forward", "pnr_sigma_geo_cat_backward")
@pytest.mark.parametrize("degree,hw", [(1, 2), (1, 16), (1, 29), (4, 2), (4, 16), (4, 29), (7, 2), (7, 16)])   # C*C + hw - 1 <= 64
@pytest.mark.parametrize("B", SH_ROWS)
def test_sigma_geo_cat(cuda, B, degree, hw):
    h, n = rnd(B + hw, B, hw), degree * degree
    arrays = dict(h=I(h), dirs=I(unit_dirs(B, B)), sigma=O(empty(B)), out=O(empty(B, n + hw - 1)))
    check(lambda a: abi("pnr_sigma_geo_cat_forward", p(a["h"]), hw, p(a["dirs"]), degree, B, p(a["sigma"]), p(a["out"])), arrays,
          f"pnr_sigma_geo_cat_forward B={B} degree={degree} hw={hw}")
    for dsigma, dout in ((True, True), (False, True), (True, False)):
        arrays = dict(h=I(h), dsigma=I(rnd(1, B)) if dsigma else None, dout=I(rnd(2, B, n + hw - 1)) if dout else None, grad_h=O(empty(B, hw)))
        check(lambda a: abi("pnr_sigma_geo_cat_backward", p(a["h"]), hw, p(a["dsigma"]), p(a["dout"]), degree, B, p(a["grad_h"])), arrays,
              f"pnr_sigma_geo_cat_backward B={B} degree={degree} hw={hw}")


# ================================================================ dense-layer weight and bias gradient
DT = {0: torch.float32, 1: torch.float16}


@guards("pnr_linear_wgrad")
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (15, 13), (31, 64), (64, 3)])
@pytest.mark.parametrize("B", [1, 255, 257])
def test_linear_wgrad(cuda, B, n_in, n_out):
    nb = nbytes_of("pnr_linear_wgrad_workspace_bytes", B, n_in, n_out)
    for xd in (0, 1):
        for yd in (0, 1):
            for acc in (0, 1):
                arrays = dict(x=I(rnd(1, B, n_in, dtype=DT[xd])), dy=I(rnd(2, B, n_out, dtype=DT[yd])), dw=O(rnd(3, n_out, n_in) if acc else empty(n_out, n_in)),
                              ws=WS(nb))
                check(lambda a: abi("pnr_linear_wgrad", p(a["x"]), xd, p(a["dy"]), yd, B, n_in, n_out, p(a["dw"]), acc, p(a["ws"]), u64(nb)), arrays,
                      f"pnr_linear_wgrad B={B} {n_in}->{n_out} dtypes {xd}{yd} accumulate={acc}")


@guards("pnr_linear_bgrad")
@pytest.mark.parametrize("n_out", [1, 13, 64, 3])
@pytest.mark.parametrize("B", [1, 255, 257])
def test_linear_bgrad(cuda, B, n_out):
    nb = nbytes_of("pnr_linear_wgrad_workspace_bytes", B, 1, n_out)
    for yd in (0, 1):
        for acc in (0, 1):
            arrays = dict(dy=I(rnd(2, B, n_out, dtype=DT[yd])), db=O(rnd(3, n_out) if acc else empty(n_out)), ws=WS(nb))
            check(lambda a: abi("pnr_linear_bgrad", p(a["dy"]), yd, B, n_out, p(a["db"]), acc, p(a["ws"]), u64(nb)), arrays,
                  f"pnr_linear_bgrad B={B} out={n_out} dtype {yd} accumulate={acc}")


# ================================================================ training composites
# Below kCoopMinSamples = 65 536 samples one thread walks a ray with kAhead = 8 samples fetched ahead, clamped to the ray's last row; from there on 16 lanes
# share a ray (csrc/composite.hip).  In both sets the last ray ends exactly at row M - 1: its clamped read-ahead is the array's last row.
T_THRESH = 1e-4
RAY_AROUND = (0, 0, 1)      # a ray triple that is valid wherever it is read: ray 0, one sample at row 0


@functools.lru_cache(maxsize=None)
def ray_set(kind):
    """small: 5 rays of 0, 1, 7, 16, 17 samples.  scan: tests/test_gpu_train_norm.py's 640-ray batch above 65 536 samples (lengths cycle through
    0, 1, 15, 16, 17, 31, 32, 33 and 200-600; rays that stop on T_thresh in lane 0 and in lane 15 of a 16-sample group), with its last ray, which
    there overruns M, ending at M - 1 here.  -> numpy arrays, read-only."""
    if kind == "small":
        rng = np.random.default_rng(5)
        counts = np.array([0, 1, 7, 16, 17])
        offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
        N, M = 5, int(counts.sum())
        rays = np.stack([rng.permutation(N), offs, counts], 1).astype(np.int32)
        sig = (rng.random(M) * 40).astype(np.float32)
        sig[offs[3]:offs[3] + 16] *= 0.03                                   # the 16-sample ray runs its full length
        dl = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], 1).astype(np.float32)
        rgb, gt = rng.random((M, 3)).astype(np.float32), rng.random((N, 3)).astype(np.float32)
    else:
        from tests.test_gpu_train_norm import batch
        b = batch("scan")
        assert any(at % 16 == 0 for at in b["forced"].values()) and any(at % 16 == 15 for at in b["forced"].values())
        N, M, sig, dl, rgb, gt = b["N"], b["M"], b["sig"], b["dl"], b["rgb"], b["gt"]
        rays = b["rays"].copy()
        rays[b["over"], 2] = 17
        assert M >= 1 << 16
    assert int(rays[-1, 1] + rays[-1, 2]) == M and int((rays[:, 1] + rays[:, 2]).max()) == M
    rng = np.random.default_rng(6)
    out = dict(N=N, M=M, rays=rays, sig=sig, dl=dl, rgb=rgb, gt=gt, gws=rng.standard_normal(N).astype(np.float32),
               gimg=rng.standard_normal((N, 3)).astype(np.float32), gnorm=rng.standard_normal(N).astype(np.float32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()      # (a copy: the shared arrays are read-only)


@guards("pnr_composite_rays_train_forward", "pnr_composite_rays_train_backward", "pnr_composite_rays_train_norm_forward",
        "pnr_composite_rays_train_norm_backward")
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["small", "scan"])
def test_composite_rays_train(cuda, kind, norm):
    b = ray_set(kind)
    N, M = b["N"], b["M"]
    ins = dict(sigmas=I(dev(b["sig"])), rgbs=I(dev(b["rgb"])), deltas=I(dev(b["dl"])), rays=I(dev(b["rays"]), around=RAY_AROUND))
    outs = dict(weights_sum=O(empty(N)), depth=O(empty(N)), image=O(empty(N, 3)))
    if norm:
        ins["rays_gt"], outs["rgb_norm"] = I(dev(b["gt"])), O(empty(N))

        def fwd(a):
            return abi("pnr_composite_rays_train_norm_forward", p(a["sigmas"]), p(a["rgbs"]), p(a["deltas"]), p(a["rays"]), p(a["rays_gt"]), M, N, T_THRESH,
                       p(a["weights_sum"]), p(a["depth"]), p(a["image"]), p(a["rgb_norm"]))
    else:
        def fwd(a):
            return abi("pnr_composite_rays_train_forward", p(a["sigmas"]), p(a["rgbs"]), p(a["deltas"]), p(a["rays"]), M, N, T_THRESH, p(a["weights_sum"]),
                       p(a["depth"]), p(a["image"]))
    ref, _ = check(fwd, {**ins, **outs}, f"composite_rays_train forward {kind} norm={norm}")
    ins.update(grad_weights_sum=I(dev(b["gws"])), grad_image=I(dev(b["gimg"])), weights_sum=I(ref["weights_sum"]), image=I(ref["image"]))
    outs = dict(grad_sigmas=O(torch.zeros(M, device="cuda")), grad_rgbs=O(torch.zeros(M, 3, device="cuda")))      # zeros_like, as raymarching.py
    if norm:
        ins.update(grad_rgb_norm=I(dev(b["gnorm"])), rgb_norm=I(ref["rgb_norm"]))

        def bwd(a):
            return abi("pnr_composite_rays_train_norm_backward", p(a["grad_weights_sum"]), p(a["grad_image"]), p(a["grad_rgb_norm"]), p(a["sigmas"]),
                       p(a["rgbs"]), p(a["deltas"]), p(a["rays"]), p(a["rays_gt"]), p(a["weights_sum"]), p(a["image"]), p(a["rgb_norm"]), M, N, T_THRESH,
                       p(a["grad_sigmas"]), p(a["grad_rgbs"]))
    else:
        def bwd(a):
            return abi("pnr_composite_rays_train_backward", p(a["grad_weights_sum"]), p(a["grad_image"]), p(a["sigmas"]), p(a["rgbs"]), p(a["deltas"]),
                       p(a["rays"]), p(a["weights_sum"]), p(a["image"]), M, N, T_THRESH, p(a["grad_sigmas"]), p(a["grad_rgbs"]))
    check(bwd, {**ins, **outs}, f"composite_rays_train backward {kind} norm={norm}")


@guards("pnr_composite_rays_flex_train_forward", "pnr_composite_rays_flex_train_backward", "pnr_spread_ray_to_sample")
@pytest.mark.parametrize("n_channel", [1, 3, 33, 128])
@pytest.mark.parametrize("kind", ["small", "scan"])
def test_composite_rays_flex_train_and_spread(cuda, kind, n_channel):
    b = ray_set(kind)
    N, M = b["N"], b["M"]
    nan_row = lambda t: torch.cat([t, torch.full((1, *t.shape[1:]), float("nan"), device="cuda")])  # noqa: E731
    # The flex kernels take a ray with offset + num_steps >= M for empty ('>=' here, '>' in the rgb kernels: the reference's quirk), so with M rows the set's
    # last ray is skipped.  spare = 1: the same rays with M + 1 rows -- the last ray is live, its last row is the last row a ray may own, and the one row behind
    # it, which no ray owns, is NaN in every input of both calls: nothing of it may reach an output, and the backward must leave its zeros alone.
    for spare in (0, 1):
        Ms = M + spare
        rows = nan_row if spare else (lambda t: t)
        ins = dict(sigmas=I(rows(dev(b["sig"]))), input=I(rows(uni(n_channel, M, n_channel))), deltas=I(rows(dev(b["dl"]))), rays=I(dev(b["rays"]), around=RAY_AROUND))
        what = f"{kind} {n_channel} rows={Ms}"
        ref, _ = check(lambda a: abi("pnr_composite_rays_flex_train_forward", p(a["sigmas"]), p(a["input"]), p(a["deltas"]), p(a["rays"]), Ms, N, n_channel,
                                     T_THRESH, p(a["output"])), {**ins, "output": O(empty(N, n_channel))}, "flex_train forward " + what)
        last = int(b["rays"][-1, 0])
        assert nans(ref["output"]) == 0 and bool((ref["output"][last] != 0).any()) == bool(spare)      # the last ray: composited, or empty
        ins.update(grad_output=I(rnd(1, N, n_channel)), output=I(ref["output"]))
        ref, _ = check(lambda a: abi("pnr_composite_rays_flex_train_backward", p(a["grad_output"]), p(a["sigmas"]), p(a["input"]), p(a["deltas"]), p(a["rays"]),
                                     p(a["output"]), Ms, N, n_channel, T_THRESH, p(a["grad_input"])),
                       {**ins, "grad_input": O(torch.zeros(Ms, n_channel, device="cuda"))}, "flex_train backward " + what)
        assert nans(ref["grad_input"]) == 0
        if spare:
            assert not bool(ref["grad_input"][-1].any())                        # the row no ray owns
            assert kind != "scan" or bool(ref["grad_input"][-2].any())          # the last ray's last row (that ray is translucent: it never stops early)
    arrays = dict(input=I(rnd(2, N, n_channel)), rays=I(dev(b["rays"]), around=RAY_AROUND), output=O(empty(M, n_channel)))
    check(lambda a: abi("pnr_spread_ray_to_sample", p(a["input"]), p(a["rays"]), M, N, n_channel, p(a["output"])), arrays,
          f"pnr_spread_ray_to_sample {kind} {n_channel}")


# ================================================================ training MLPs: 32-row wave tiles, 128-row workgroups, 16-byte requests (csrc/mlp.hip)
MLP_ROWS = (1, 31, 32, 33, 127, 128, 129, 161)
MLP_STACKS = {"3-64-15": ((3, 64, 15), 0), "35-64-3-sigmoid": ((35, 64, 3), _lib.MLP_OUT_SIGMOID), "15-64-64-13": ((15, 64, 64, 13), 0),
              "32-64-64-16": ((32, 64, 64, 16), 1), "33-64-64-7": ((33, 64, 64, 7), 0)}


def mlp_desc(dims, act):
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    d.activation = act
    return d


def mlp_packed(desc, dims, seed=0):
    """(weights, packed blob on plain tensors)"""
    ws = [rnd(seed + l, dims[l + 1], dims[l], scale=0.3) for l in range(len(dims) - 1)]
    packed = torch.zeros(nbytes_of("pnr_mlp_packed_bytes", ctypes.byref(desc)) // 4, device="cuda")      # (a two-layer stack leaves the third scale slot alone)
    assert abi("pnr_mlp_pack", ctypes.byref(desc), p(ws[0]), p(ws[1]), p(ws[2]) if len(ws) == 3 else None, p(packed)) == 0
    return ws, packed


@guards("pnr_mlp_pack")
@pytest.mark.parametrize("stack", list(MLP_STACKS))
def test_mlp_pack(cuda, stack):
    dims, act = MLP_STACKS[stack]
    desc = mlp_desc(dims, act)
    ws, packed = mlp_packed(desc, dims)
    arrays = {f"w{l}": I(w) for l, w in enumerate(ws)}
    arrays["packed"] = O(torch.zeros_like(packed), weak=16)      # exactly pnr_mlp_packed_bytes
    ref, _ = check(lambda a: abi("pnr_mlp_pack", ctypes.byref(desc), p(a["w0"]), p(a["w1"]), p(a.get("w2")), p(a["packed"])), arrays, f"pnr_mlp_pack {stack}")
    assert same_bits(ref["packed"], packed)


@guards("pnr_mlp_forward", "pnr_mlp_backward", "pnr_mlp_forward_lm", "pnr_mlp_backward_lm")
@pytest.mark.parametrize("f16x3", [1, 0])
@pytest.mark.parametrize("stack", list(MLP_STACKS))
def test_mlp_forward_and_backward(cuda, stack, f16x3):
    dims, act = MLP_STACKS[stack]
    desc, n = mlp_desc(dims, act), len(dims) - 1
    sig = bool(act & _lib.MLP_OUT_SIGMOID)
    with option("mlp_f16x3", f16x3, 1):
        ws, packed = mlp_packed(desc, dims)
        for B in MLP_ROWS:
            what = f"{stack} B={B} mlp_f16x3={f16x3}"
            x, dy = rnd(B, B, dims[0]), rnd(B + 1, B, dims[-1])
            nb = nbytes_of("pnr_mlp_backward_workspace_bytes", ctypes.byref(desc), B)
            refused = ERR_ALIGNMENT if B * min(dims[0], dims[-1]) < 4 else 0      # fewer than four floats in an activation array: documented as refused

            def fwd(a):
                return abi("pnr_mlp_forward", ctypes.byref(desc), p(a["packed"]), p(a["x"]), B, p(a["y"]))

            def bwd(a):
                return abi("pnr_mlp_backward", ctypes.byref(desc), p(a["packed"]), p(a["x"]), p(a["y"]), p(a["dy"]), B, p(a["dx"]), p(a["dw0"]), p(a["dw1"]),
                           p(a.get("dw2")), p(a["ws"]), u64(nb))

            f_arrays = dict(packed=I(packed, weak=16), x=I(x, weak=16), y=O(empty(B, dims[-1]), weak=16))
            ref, _ = check(fwd, f_arrays, "pnr_mlp_forward " + what, expect=refused)
            y = ref["y"] if ref is not None else empty(B, dims[-1])
            b_arrays = dict(packed=I(packed, weak=16), x=I(x, weak=16), y=I(y, weak=16) if sig else None, dy=I(dy, weak=16), dx=O(empty(B, dims[0]), weak=16),
                            ws=WS(nb), **{f"dw{l}": O(empty(dims[l + 1], dims[l])) for l in range(n)})
            check(bwd, b_arrays, "pnr_mlp_backward " + what, expect=refused)
            if not refused:     # an activation array that starts 4 bytes behind a 16-byte boundary is refused, and nothing is written
                check(fwd, f_arrays, "pnr_mlp_forward misaligned " + what, expect=ERR_ALIGNMENT, modes=(4,))
                check(bwd, b_arrays, "pnr_mlp_backward misaligned " + what, expect=ERR_ALIGNMENT, modes=(4,))
            if dims[0] < 32:
                continue
            # the level-major forms: the first 32 columns from enc [16, B, 2], the rest from x_tail [B, dims[0] - 32]
            tail = dims[0] - 32
            enc, x_tail = rnd(B + 2, 16, B, 2), (rnd(B + 3, B, tail) if tail else None)
            refused = ERR_ALIGNMENT if B * min([dims[0], dims[-1]] + ([tail] if tail else [])) < 4 else 0
            if tail == 1:
                refused = ERR_UNSUPPORTED       # a one-column x_tail has no 32-bit reciprocal (include/pnr.h): refused, not staged into row 0

            def fwd_lm(a):
                return abi("pnr_mlp_forward_lm", ctypes.byref(desc), p(a["packed"]), p(a["enc"]), 16, p(a["x_tail"]), B, p(a["y"]))

            def bwd_lm(a):
                return abi("pnr_mlp_backward_lm", ctypes.byref(desc), p(a["packed"]), p(a["enc"]), 16, p(a["x_tail"]), p(a["dy"]), B, p(a["denc"]), p(a["dw0"]),
                           p(a["dw1"]), p(a.get("dw2")), p(a["ws"]), u64(nb))

            f_arrays = dict(packed=I(packed, weak=16), enc=I(enc, weak=16), x_tail=I(x_tail, weak=16) if tail else None, y=O(empty(B, dims[-1]), weak=16))
            check(fwd_lm, f_arrays, "pnr_mlp_forward_lm " + what, expect=refused)
            if not refused:
                check(fwd_lm, f_arrays, "pnr_mlp_forward_lm misaligned " + what, expect=ERR_ALIGNMENT, modes=(4,))
            if sig:
                continue        # pnr_mlp_backward_lm refuses a sigmoid output: no stack behind an encoder ends in one
            b_arrays = dict(packed=I(packed, weak=16), enc=I(enc, weak=16), x_tail=I(x_tail, weak=16) if tail else None, dy=I(dy, weak=16),
                            denc=O(empty(16, B, 2), weak=16), ws=WS(nb), **{f"dw{l}": O(empty(dims[l + 1], dims[l])) for l in range(n)})
            check(bwd_lm, b_arrays, "pnr_mlp_backward_lm " + what, expect=refused)
            if not refused:
                check(bwd_lm, b_arrays, "pnr_mlp_backward_lm misaligned " + what, expect=ERR_ALIGNMENT, modes=(4,))


@guards("pnr_mlp_forward", "pnr_mlp_backward")
@pytest.mark.parametrize("dims", [(1, 64, 15), (15, 64, 1), (1, 64, 64, 1)])
def test_mlp_refuses_a_one_column_end(cuda, dims):
    desc, n, B = mlp_desc(dims, 0), len(dims) - 1, 33
    ws, packed = mlp_packed(desc, dims)
    nb = nbytes_of("pnr_mlp_backward_workspace_bytes", ctypes.byref(desc), B)
    arrays = dict(packed=I(packed, weak=16), x=I(rnd(1, B, dims[0]), weak=16), y=O(empty(B, dims[-1]), weak=16))
    check(lambda a: abi("pnr_mlp_forward", ctypes.byref(desc), p(a["packed"]), p(a["x"]), B, p(a["y"])), arrays, f"pnr_mlp_forward {dims}", expect=ERR_UNSUPPORTED)
    arrays = dict(packed=I(packed, weak=16), x=I(rnd(1, B, dims[0]), weak=16), dy=I(rnd(2, B, dims[-1]), weak=16), dx=O(empty(B, dims[0]), weak=16), ws=WS(nb),
                  **{f"dw{l}": O(empty(dims[l + 1], dims[l])) for l in range(n)})
    check(lambda a: abi("pnr_mlp_backward", ctypes.byref(desc), p(a["packed"]), p(a["x"]), None, p(a["dy"]), B, p(a["dx"]), p(a["dw0"]), p(a["dw1"]), p(a.get("dw2")),
                        p(a["ws"]), u64(nb)), arrays, f"pnr_mlp_backward {dims}", expect=ERR_UNSUPPORTED)


# ================================================================ hash grid
SHIPPED = dict(D=3, C=2, L=16, H=16, pls=float(np.exp2(np.log2(2048 / 16) / 15)), log2T=19)
GRID_ROWS = (1, 63, 64, 65, 257)


def small_geometry(D, C):
    return dict(D=D, C=C, L=4, H=16, pls=2.0, log2T=12)


def grid_offsets(g, ac):
    from palettenerf_amd.gridencoder import level_offsets
    return level_offsets(g["D"], g["L"], g["pls"], g["H"], g["log2T"], ac)


def grid_inputs(B, D, seed):
    """uniform in [0, 1), with rows at exactly 0.0 and exactly 1.0 and rows outside [0, 1]"""
    x = uni(seed, B, D).cpu().numpy()
    x[0] = 1.0
    if B >= 8:
        x[1] = 0.0
        x[2, 0], x[3, D - 1], x[4, 0], x[5, D - 1] = 1.0, 0.0, -0.25, 1.5
    return x


def table_grad_close(g, x, offsets, ac, gridtype, grad_rows, u):
    """Both calls' grad_embeddings against the float64 table gradient under tests/grid_reference.py's table_grad_bound; rows no sample reaches stay 0."""
    ref = gr.GridReference(x, offsets, g["pls"], g["H"], gridtype, ac)
    touched, want, mag, n = ref.table_grad_sparse(grad_rows)
    bound = gr.table_grad_bound(g["D"], mag, n, u)
    idx = torch.from_numpy(touched).cuda()

    def close(got, plain):
        for name, t in (("guarded", got), ("plain", plain)):
            ratio = gr.error_ratio(t[idx].double().cpu().numpy(), want, bound)
            assert ratio <= 1.0, f"grad_embeddings ({name} call): {ratio} of table_grad_bound"
            rest = t.clone()
            rest[idx] = 0
            assert not bool(rest.any()), f"grad_embeddings ({name} call): a row no sample reaches was written"
    return close


def grid_cases():
    cases = []
    for gridtype in (0, 1):
        for dtype in (0, 1):
            cases.append(pytest.param(SHIPPED, gridtype, dtype, id=f"shipped-{'tiled' if gridtype else 'hash'}-{'fp16' if dtype else 'fp32'}"))
    for D, C in ((2, 1), (3, 4), (3, 8)):
        cases.append(pytest.param(small_geometry(D, C), 0, 0, id=f"D{D}C{C}-hash-fp32"))
    return cases


@guards("pnr_grid_encode_forward", "pnr_grid_encode_forward_layout", "pnr_grid_encode_backward")
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("g,gridtype,dtype", grid_cases())
def test_grid_encode(cuda, g, gridtype, dtype, ac):
    D, C, L, H, S = g["D"], g["C"], g["L"], g["H"], float(np.log2(g["pls"]))
    offsets = grid_offsets(g, ac)
    rows, td, u = int(offsets[-1]), DT[dtype], (gr.U16 if dtype else gr.U32)
    wk = 4 if dtype else None      # fp16 arrays move as pairs of halves: include/pnr.h names 4 bytes as their weakest start; 2 bytes is refused (below)

    def on_odd_half(arrays):
        """the same arrays with every fp16 one starting 2 bytes behind a 256-byte boundary"""
        return {k: (Arr(v.role, v.t, v.around, 2) if v is not None and v.t is not None and v.t.dtype == torch.float16 else v) for k, v in arrays.items()}
    table = (uni(1, rows, C) - 0.5).to(td)                     # exactly offsets[L] * C elements
    off = I(dev(offsets), around=(int(offsets[-1]),))
    for B in GRID_ROWS:
        x = grid_inputs(B, D, B)
        for with_dy in (False, True):
            what = f"{g} gridtype={gridtype} dtype={dtype} ac={ac} B={B} dy_dx={with_dy}"
            arrays = dict(inputs=I(dev(x)), embeddings=I(table, weak=wk), offsets=off, outputs=O(empty(L, B, C, dtype=td), weak=wk),
                          dy_dx=O(empty(B, L * D * C, dtype=td), weak=wk) if with_dy else None)
            ref, _ = check(lambda a: abi("pnr_grid_encode_forward", p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["outputs"]), B, D, C, L, S, H,
                                         p(a["dy_dx"]), gridtype, int(ac), dtype), arrays, "pnr_grid_encode_forward " + what)
            if dtype and B == GRID_ROWS[-1]:
                check(lambda a: abi("pnr_grid_encode_forward", p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["outputs"]), B, D, C, L, S, H, p(a["dy_dx"]),
                                    gridtype, int(ac), dtype), on_odd_half(arrays), "pnr_grid_encode_forward on an odd half " + what, expect=ERR_ALIGNMENT, modes=("weak",))
            for layout in ((0, 1) if (D, C, with_dy) == (3, 2, False) else (0,)):
                arrays["outputs"] = O(empty(*((B, L * C) if layout else (L, B, C)), dtype=td), weak=wk)
                lay, _ = check(lambda a: abi("pnr_grid_encode_forward_layout", p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["outputs"]), B, D, C, L, S,
                                             H, p(a["dy_dx"]), gridtype, int(ac), dtype, layout), arrays, f"pnr_grid_encode_forward_layout {layout} " + what)
                assert same_bits(lay["outputs"].view(B, L, C).permute(1, 0, 2).contiguous() if layout else lay["outputs"], ref["outputs"])
            grad_rows = rnd(B + 9, B, L * C).to(td)
            grad = grad_rows.view(B, L, C).permute(1, 0, 2).contiguous()
            arrays = dict(grad=I(grad, weak=wk), inputs=I(dev(x)), embeddings=I(table, weak=wk), offsets=off, grad_embeddings=O(torch.zeros(rows, C, dtype=td, device="cuda"), weak=wk),
                          dy_dx=I(ref["dy_dx"], weak=wk) if with_dy else None, grad_inputs=O(torch.zeros(B, D, dtype=td, device="cuda"), weak=wk) if with_dy else None)
            close = table_grad_close(g, x, offsets, ac, gridtype, grad_rows.float().cpu().numpy(), u)
            check(lambda a: abi("pnr_grid_encode_backward", p(a["grad"]), p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["grad_embeddings"]), B, D, C, L,
                                S, H, p(a["dy_dx"]), p(a["grad_inputs"]), gridtype, int(ac), dtype), arrays, "pnr_grid_encode_backward " + what,
                  close={"grad_embeddings": close})
            if dtype and B == GRID_ROWS[-1]:     # the 4-byte atomic of a pair of halves never runs on a table that starts on an odd half
                check(lambda a: abi("pnr_grid_encode_backward", p(a["grad"]), p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["grad_embeddings"]), B, D, C, L,
                                    S, H, p(a["dy_dx"]), p(a["grad_inputs"]), gridtype, int(ac), dtype), on_odd_half(arrays),
                      "pnr_grid_encode_backward on an odd half " + what, expect=ERR_ALIGNMENT, modes=("weak",))


@guards("pnr_grid_encode_forward")
@pytest.mark.parametrize("grid_nt", [1, 2, 3])
def test_grid_encode_forward_nontemporal_options(cuda, grid_nt):
    g, S = SHIPPED, float(np.log2(SHIPPED["pls"]))
    offsets = grid_offsets(g, False)
    table = uni(1, int(offsets[-1]), 2) - 0.5
    with option("grid_nt", grid_nt, 0):
        for B in GRID_ROWS:
            arrays = dict(inputs=I(dev(grid_inputs(B, 3, B))), embeddings=I(table), offsets=I(dev(offsets), around=(int(offsets[-1]),)), outputs=O(empty(16, B, 2)))
            check(lambda a: abi("pnr_grid_encode_forward", p(a["inputs"]), p(a["embeddings"]), p(a["offsets"]), p(a["outputs"]), B, 3, 2, 16, S, 16, None, 0, 0, 0),
                  arrays, f"pnr_grid_encode_forward grid_nt={grid_nt} B={B}")


@guards("pnr_grid_encode_forward_pair", "pnr_grid_encode_backward_binned")
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("gridtype", [0, 1])
def test_grid_pair_lookup_and_binned_table_gradient(cuda, gridtype, ac):
    g, S = SHIPPED, float(np.log2(SHIPPED["pls"]))
    offsets = grid_offsets(g, ac)
    rows = int(offsets[-1])
    t0, t1 = uni(1, rows, 2) - 0.5, uni(2, rows, 2) - 0.5
    pair = torch.cat([t0, t1], dim=1).contiguous()                # [row][table 0 | table 1][2]
    off = I(dev(offsets), around=(rows,))
    for B in GRID_ROWS:
        x = grid_inputs(B, 3, B)
        what = f"gridtype={gridtype} ac={ac} B={B}"
        arrays = dict(inputs=I(dev(x)), pair=I(pair, weak=16), offsets=off, out0=O(empty(16, B, 2)), out1=O(empty(16, B, 2)))
        ref, _ = check(lambda a: abi("pnr_grid_encode_forward_pair", p(a["inputs"]), p(a["pair"]), p(a["offsets"]), p(a["out0"]), p(a["out1"]), B, 16, S, 16,
                                     gridtype, int(ac)), arrays, "pnr_grid_encode_forward_pair " + what)
        for k, t in enumerate((t0, t1)):
            one = empty(16, B, 2)
            assert abi("pnr_grid_encode_forward", p(dev(x)), p(t), p(off.t), p(one), B, 3, 2, 16, S, 16, None, gridtype, int(ac), 0) == 0
            assert same_bits(ref[f"out{k}"], one)
        nb = nbytes_of("pnr_grid_backward_binned_workspace_bytes", B, 16, rows)
        grad_rows = rnd(B + 9, B, 32)
        arrays = dict(grad=I(grad_rows.view(B, 16, 2).permute(1, 0, 2).contiguous()), inputs=I(dev(x)), offsets=off,
                      grad_embeddings=O(torch.zeros(rows, 2, device="cuda")), ws=WS(nb))
        close = table_grad_close(g, x, offsets, ac, gridtype, grad_rows.cpu().numpy(), gr.U32)
        check(lambda a: abi("pnr_grid_encode_backward_binned", p(a["grad"]), p(a["inputs"]), p(a["offsets"]), p(a["grad_embeddings"]), B, 3, 2, 16, S, 16, gridtype,
                            int(ac), u64(rows), p(a["ws"]), u64(nb)), arrays, "pnr_grid_encode_backward_binned " + what, close={"grad_embeddings": close})


# ================================================================ inference march and composites, scene S0 (256 rays per workgroup, n_step <= 8)
BOUND, CASCADE, GRID_H, MAX_STEPS = 2.0, 2, 128, 1024


@functools.lru_cache(maxsize=None)
def scene_s0():
    """Scene S0 (scene.brick_density_grid) and the 1024 rays of a 32 x 32 frame of it, on the device; read-only by convention."""
    from palettenerf_amd import raymarching, scene
    grid = dev(scene.brick_density_grid())
    bitfield = dev(scene.packbits_np(scene.brick_density_grid(), 0.5))
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(32, 32), 32, 32)
    ro, rd = ro[0].contiguous().cuda(), rd[0].contiguous().cuda()
    aabb = torch.tensor([-2, -2, -2, 2, 2, 2], dtype=torch.float32, device="cuda")
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    mip = torch.zeros(nbytes_of("pnr_occupancy_mip_bytes", CASCADE, GRID_H), dtype=torch.uint8, device="cuda")
    assert abi("pnr_build_occupancy_mip", p(bitfield), CASCADE, GRID_H, BOUND, p(mip)) == 0
    torch.cuda.synchronize()
    return dict(grid=grid, bitfield=bitfield, ro=ro, rd=rd, aabb=aabb, nears=nears, fars=fars, mip=mip)


def central_rays(n):
    """ids of n rays of the 32 x 32 frame, the frame's centre (where the scene is) first"""
    yy, xx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    order = np.argsort(np.maximum(np.abs(yy - 15.5), np.abs(xx - 15.5)).reshape(-1), kind="stable")
    return order[:n]


@guards("pnr_near_far_from_aabb", "pnr_sph_from_ray", "pnr_packbits", "pnr_morton3d", "pnr_morton3d_invert", "pnr_build_occupancy_mip")
@pytest.mark.parametrize("N", [1, 65, 130])
def test_ray_and_grid_utilities(cuda, N):
    s = scene_s0()
    ids = torch.from_numpy(central_rays(N)).cuda()
    arrays = dict(rays_o=I(s["ro"][ids].contiguous()), rays_d=I(s["rd"][ids].contiguous()), aabb=I(s["aabb"]), nears=O(empty(N)), fars=O(empty(N)))
    check(lambda a: abi("pnr_near_far_from_aabb", p(a["rays_o"]), p(a["rays_d"]), p(a["aabb"]), N, 0.2, p(a["nears"]), p(a["fars"])), arrays,
          f"pnr_near_far_from_aabb N={N}")
    arrays = dict(rays_o=I(s["ro"][ids].contiguous()), rays_d=I(s["rd"][ids].contiguous()), coords=O(empty(N, 2)))
    check(lambda a: abi("pnr_sph_from_ray", p(a["rays_o"]), p(a["rays_d"]), 4.0, N, p(a["coords"])), arrays, f"pnr_sph_from_ray N={N}")
    for nbytes in (N, s["bitfield"].numel()):          # N bytes of the bitfield from 8 N cells, and the whole grid
        arrays = dict(grid=I(s["grid"].view(-1)[:8 * nbytes].contiguous()), bitfield=O(torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), weak=1))
        ref, _ = check(lambda a: abi("pnr_packbits", p(a["grid"]), nbytes, 0.5, p(a["bitfield"])), arrays, f"pnr_packbits {nbytes} bytes")
        assert torch.equal(ref["bitfield"], s["bitfield"][:nbytes])
    coords = torch.randint(0, GRID_H, (N, 3), generator=torch.Generator().manual_seed(N), dtype=torch.int32).cuda()
    arrays = dict(coords=I(coords, around=(0, 0, 0)), indices=O(torch.zeros(N, dtype=torch.int32, device="cuda")))
    ref, _ = check(lambda a: abi("pnr_morton3d", p(a["coords"]), N, p(a["indices"])), arrays, f"pnr_morton3d N={N}")
    arrays = dict(indices=I(ref["indices"], around=(0,)), coords=O(torch.zeros(N, 3, dtype=torch.int32, device="cuda")))
    ref, _ = check(lambda a: abi("pnr_morton3d_invert", p(a["indices"]), N, p(a["coords"])), arrays, f"pnr_morton3d_invert N={N}")
    assert torch.equal(ref["coords"], coords)
    if N == 1:      # the mip at exactly pnr_occupancy_mip_bytes; the bitfield on an 8-byte boundary, as the header requires
        arrays = dict(grid=I(s["bitfield"], around=0x00, weak=8), mip=O(torch.zeros_like(s["mip"]), weak=8))
        ref, _ = check(lambda a: abi("pnr_build_occupancy_mip", p(a["grid"]), CASCADE, GRID_H, BOUND, p(a["mip"])), arrays, "pnr_build_occupancy_mip")
        assert torch.equal(ref["mip"], s["mip"])


def alive_set(n_alive, n_step):
    """The state of a march iteration: n_alive rays of the frame (a permutation of the central ones), rows padded as raymarching.march_rays pads
    them (to the next multiple of 128, always)."""
    s = scene_s0()
    ids = np.random.default_rng(n_alive).permutation(central_rays(n_alive)).astype(np.int32)
    M = n_alive * n_step
    M += 128 - M % 128
    return s, dev(ids), M


@guards("pnr_march_rays", "pnr_march_rays_mip", "pnr_march_rays_fill")
@pytest.mark.parametrize("n_step", [1, 8])
@pytest.mark.parametrize("n_alive", [1, 63, 65, 257])
def test_march_rays(cuda, n_alive, n_step):
    s, ids, M = alive_set(n_alive, n_step)
    common = dict(rays_alive=I(ids, around=(int(ids[0]),)), rays_t=I(s["nears"]), rays_o=I(s["ro"]), rays_d=I(s["rd"]), grid=I(s["bitfield"], around=0x00, weak=8),
                  nears=I(s["nears"]), fars=I(s["fars"]))
    zeros = lambda: dict(xyzs=O(torch.zeros(M, 3, device="cuda")), dirs=O(torch.zeros(M, 3, device="cuda")), deltas=O(torch.zeros(M, 2, device="cuda")))  # noqa: E731
    head = lambda a: (n_alive, n_step, p(a["rays_alive"]), p(a["rays_t"]), p(a["rays_o"]), p(a["rays_d"]), BOUND, 0.0, MAX_STEPS, CASCADE, GRID_H, p(a["grid"]),  # noqa: E731
                      p(a["nears"]), p(a["fars"]), p(a["xyzs"]), p(a["dirs"]), p(a["deltas"]))
    what = f"n_alive={n_alive} n_step={n_step}"
    plain, _ = check(lambda a: abi("pnr_march_rays", *head(a), p(a["noises"])), {**common, **zeros(), "noises": I(torch.zeros(n_alive, device="cuda"))},
                     "pnr_march_rays " + what)
    check(lambda a: abi("pnr_march_rays", *head(a), p(a["noises"])), {**common, **zeros(), "noises": I(uni(n_alive, n_alive))}, "pnr_march_rays jittered " + what)
    mip = I(s["mip"], around=0x00, weak=8)
    with_mip, _ = check(lambda a: abi("pnr_march_rays_mip", *head(a), None, p(a["mip"])), {**common, **zeros(), "mip": mip}, "pnr_march_rays_mip " + what)
    # uninitialised buffers, fill_rows = the rows the wrapper allocates
    raw = dict(xyzs=O(empty(M, 3)), dirs=O(empty(M, 3)), deltas=O(empty(M, 2)))
    filled, _ = check(lambda a: abi("pnr_march_rays_fill", *head(a), None, p(a["mip"]), M), {**common, **raw, "mip": mip}, "pnr_march_rays_fill " + what)
    for k in ("xyzs", "dirs", "deltas"):
        assert same_bits(with_mip[k], plain[k]) and same_bits(filled[k], plain[k]), k


@functools.lru_cache(maxsize=None)
def marched(n_alive, n_step):
    """deltas of a march iteration and a field's answers on its rows (random): what the inference composites read"""
    s, ids, M = alive_set(n_alive, n_step)
    xyzs, dirs, deltas = empty(M, 3), empty(M, 3), empty(M, 2)
    assert abi("pnr_march_rays_fill", n_alive, n_step, p(ids), p(s["nears"]), p(s["ro"]), p(s["rd"]), BOUND, 0.0, MAX_STEPS, CASCADE, GRID_H, p(s["bitfield"]),
               p(s["nears"]), p(s["fars"]), p(xyzs), p(dirs), p(deltas), None, p(s["mip"]), M) == 0
    torch.cuda.synchronize()
    sigmas = uni(n_alive, M, hi=60.0)
    sigmas[::5] *= 40          # some rays end on T_thresh inside the iteration
    return s, ids, M, deltas, sigmas


@guards("pnr_composite_rays", "pnr_composite_rays_flex", "pnr_composite_rays_flex_multi", "pnr_compact_alive")
@pytest.mark.parametrize("n_step", [1, 8])
@pytest.mark.parametrize("n_alive", [1, 63, 65, 257])
def test_inference_composites_and_compaction(cuda, n_alive, n_step):
    s, ids, M, deltas, sigmas = marched(n_alive, n_step)
    N, T, live = 1024, 1e-2, (int(ids[0]),)
    what = f"n_alive={n_alive} n_step={n_step}"
    state = dict(weights_sum=uni(1, N, hi=0.5), depth=uni(2, N), image=uni(3, N, 3))
    arrays = dict(rays_alive=IO(ids, around=live), rays_t=O(s["nears"]), sigmas=I(sigmas), rgbs=I(uni(4, M, 3)), deltas=I(deltas),
                  **{k: O(v) for k, v in state.items()})
    done, _ = check(lambda a: abi("pnr_composite_rays", n_alive, n_step, T, p(a["rays_alive"]), p(a["rays_t"]), p(a["sigmas"]), p(a["rgbs"]), p(a["deltas"]),
                                  p(a["weights_sum"]), p(a["depth"]), p(a["image"])), arrays, "pnr_composite_rays " + what)
    maps = {}
    for n_channel in (3, 12, 33):
        arrays = dict(rays_alive=I(ids, around=live), rays_t=I(s["nears"]), sigmas=I(sigmas), input=I(uni(n_channel, M, n_channel)), deltas=I(deltas),
                      weights_sum=I(state["weights_sum"]), output=O(uni(5, N, n_channel)))
        maps[n_channel] = check(lambda a: abi("pnr_composite_rays_flex", n_alive, n_step, n_channel, T, p(a["rays_alive"]), p(a["rays_t"]), p(a["sigmas"]), p(a["input"]),
                                              p(a["deltas"]), p(a["weights_sum"]), p(a["output"])), arrays, f"pnr_composite_rays_flex {n_channel} " + what)[0]["output"]
    arrays = dict(rays_alive=I(ids, around=live), rays_t=I(s["nears"]), sigmas=I(sigmas), deltas=I(deltas), weights_sum=I(state["weights_sum"]))
    for n_channel in maps:
        arrays[f"in{n_channel}"], arrays[f"out{n_channel}"] = I(uni(n_channel, M, n_channel)), O(uni(5, N, n_channel))

    def multi(a):
        table = (_lib.FlexMap * len(maps))()
        for k, n_channel in enumerate(maps):
            table[k].n_channel, table[k].input, table[k].output = n_channel, p(a[f"in{n_channel}"]), p(a[f"out{n_channel}"])
        return abi("pnr_composite_rays_flex_multi", n_alive, n_step, T, p(a["rays_alive"]), p(a["rays_t"]), p(a["sigmas"]), p(a["deltas"]), p(a["weights_sum"]), table,
                   len(maps))

    ref, _ = check(multi, arrays, "pnr_composite_rays_flex_multi " + what)
    for n_channel, want in maps.items():
        assert same_bits(ref[f"out{n_channel}"], want)
    # the list the composite left (dead rays are -1), compacted; the scratch at exactly pnr_scan_scratch_bytes
    nb = nbytes_of("pnr_scan_scratch_bytes", n_alive)
    arrays = dict(rays_alive_in=I(done["rays_alive"], around=live), rays_alive_out=O(torch.full((n_alive,), -7, dtype=torch.int32, device="cuda")),
                  n_alive_out=O(torch.full((1,), -7, dtype=torch.int32, device="cuda")), scratch=WS(nb))
    ref, _ = check(lambda a: abi("pnr_compact_alive", n_alive, p(a["rays_alive_in"]), p(a["rays_alive_out"]), p(a["n_alive_out"]), p(a["scratch"])), arrays,
                   "pnr_compact_alive " + what)
    kept = done["rays_alive"][done["rays_alive"] >= 0]
    assert int(ref["n_alive_out"]) == kept.numel() and torch.equal(ref["rays_alive_out"][:kept.numel()], kept)


@guards("pnr_march_rays_train", "pnr_march_rays_train_mip")
@pytest.mark.parametrize("N", [1, 65, 130])
def test_march_rays_train(cuda, N):
    s = scene_s0()
    ids = torch.from_numpy(central_rays(N)).cuda()
    M, nb = N * MAX_STEPS, nbytes_of("pnr_scan_scratch_bytes", N)
    common = dict(rays_o=I(s["ro"][ids].contiguous()), rays_d=I(s["rd"][ids].contiguous()), grid=I(s["bitfield"], around=0x00, weak=8), nears=I(s["nears"][ids].contiguous()),
                  fars=I(s["fars"][ids].contiguous()), noises=I(uni(N, N)))
    outs = lambda: dict(xyzs=O(empty(M, 3)), dirs=O(empty(M, 3)), deltas=O(empty(M, 2)), rays=O(torch.zeros(N, 3, dtype=torch.int32, device="cuda")),  # noqa: E731
                        counter=O(torch.zeros(2, dtype=torch.int32, device="cuda")), scratch=WS(nb))
    head = lambda a: (p(a["rays_o"]), p(a["rays_d"]), p(a["grid"]), BOUND, 0.0, MAX_STEPS, N, CASCADE, GRID_H, M, p(a["nears"]), p(a["fars"]), p(a["xyzs"]),  # noqa: E731
                      p(a["dirs"]), p(a["deltas"]), p(a["rays"]), p(a["counter"]), p(a["noises"]), p(a["scratch"]))
    plain, _ = check(lambda a: abi("pnr_march_rays_train", *head(a)), {**common, **outs()}, f"pnr_march_rays_train N={N}")
    assert int(plain["counter"][1]) == N and int(plain["counter"][0]) > 0
    mip = I(s["mip"], around=0x00, weak=8)
    for t_store in (False, True):
        arrays = {**common, **outs(), "mip": mip, "t_store": O(empty(N * MAX_STEPS)) if t_store else None}
        # (t_store is scratch: what the counting pass leaves there is compared like an output all the same)
        ref, _ = check(lambda a: abi("pnr_march_rays_train_mip", *head(a), p(a["mip"]), p(a["t_store"])), arrays, f"pnr_march_rays_train_mip N={N} t_store={t_store}")
        m = int(plain["counter"][0])
        assert torch.equal(ref["rays"], plain["rays"]) and torch.equal(ref["counter"], plain["counter"])
        for k in ("xyzs", "dirs", "deltas"):
            assert same_bits(ref[k][:m], plain[k][:m]), k


# ================================================================ PaletteNeRF training: heads, shade, smooth loss, ray-level loss
PAL_ROWS = (1, 63, 64, 65, 257)
PAL_BASES = (1, 4, 10)
PAL_CLIPS = (0, 16, 32)


@guards("pnr_palette_heads_forward", "pnr_palette_heads_backward")
@pytest.mark.parametrize("in_dim", [15, 16])
@pytest.mark.parametrize("nb", PAL_BASES)
def test_palette_heads(cuda, nb, in_dim):
    n_or = 3 * nb + 1
    w_or, b_or, w_om = rnd(1, n_or, in_dim, scale=0.3), rnd(2, n_or, scale=0.3), rnd(3, nb, in_dim, scale=0.3)
    for M in PAL_ROWS:
        h = rnd(M, M, in_dim)
        arrays = dict(h=I(h), w_or=I(w_or), b_or=I(b_or), w_om=I(w_om), offsets_radiance=O(empty(M, n_or)), omega=O(empty(M, nb)))
        check(lambda a: abi("pnr_palette_heads_forward", p(a["h"]), p(a["w_or"]), p(a["b_or"]), p(a["w_om"]), M, nb, in_dim, p(a["offsets_radiance"]), p(a["omega"])),
              arrays, f"pnr_palette_heads_forward M={M} nb={nb} in={in_dim}")
        for want_h in (True, False):
            arrays = dict(h=I(h), w_or=I(w_or), w_om=I(w_om), g_or=I(rnd(4, M, n_or)), g_om=I(rnd(5, M, nb)), grad_h=O(empty(M, in_dim)) if want_h else None,
                          grad_pre=O(empty(M, n_or + nb)))
            check(lambda a: abi("pnr_palette_heads_backward", p(a["h"]), p(a["w_or"]), p(a["w_om"]), p(a["g_or"]), p(a["g_om"]), M, nb, in_dim, p(a["grad_h"]),
                                p(a["grad_pre"])), arrays, f"pnr_palette_heads_backward M={M} nb={nb} in={in_dim} grad_h={want_h}")


@guards("pnr_palette_train_shade_forward", "pnr_palette_train_shade_backward")
@pytest.mark.parametrize("clip_dim", PAL_CLIPS)
@pytest.mark.parametrize("nb", PAL_BASES)
def test_palette_train_shade(cuda, nb, clip_dim):
    n_or, n_all = 3 * nb + 1, 13 + clip_dim + nb
    nbytes = nbytes_of("pnr_palette_train_shade_workspace_bytes", nb)
    basis_color = uni(9, nb, 3, lo=-0.2, hi=1.2)          # the unclamped parameter
    for M in PAL_ROWS:
        ins = dict(omega=I(uni(1, M, nb)), offsets_radiance=I(rnd(2, M, n_or, scale=0.3)), view_dep=I(rnd(3, M, 3, scale=0.1)), basis_color=I(basis_color))
        arrays = dict(**ins, diffuse=I(uni(4, M, 3)), clip_feat=I(rnd(5, M, clip_dim)) if clip_dim else None, smooth_norm=I(uni(6, M)), rgbs=O(empty(M, 3)),
                      all_buffer=O(empty(M, n_all)))
        check(lambda a: abi("pnr_palette_train_shade_forward", M, nb, clip_dim, p(a["omega"]), p(a["offsets_radiance"]), p(a["view_dep"]), p(a["diffuse"]),
                            p(a["clip_feat"]), p(a["smooth_norm"]), p(a["basis_color"]), p(a["rgbs"]), p(a["all_buffer"])), arrays,
              f"pnr_palette_train_shade_forward M={M} nb={nb} clip={clip_dim}")
        for optional in (True, False):
            arrays = dict(**ins, grad_rgbs=I(rnd(7, M, 3)), grad_all=I(rnd(8, M, n_all)), grad_omega=O(empty(M, nb)), grad_or=O(empty(M, n_or)),
                          grad_view_dep=O(empty(M, 3)), grad_diffuse=O(empty(M, 3)), grad_clip_feat=O(empty(M, clip_dim)) if optional and clip_dim else None,
                          grad_smooth_norm=O(empty(M)) if optional else None, grad_basis_color=O(empty(nb, 3)) if optional else None, ws=WS(nbytes))
            check(lambda a: abi("pnr_palette_train_shade_backward", M, nb, clip_dim, p(a["omega"]), p(a["offsets_radiance"]), p(a["view_dep"]), p(a["basis_color"]),
                                p(a["grad_rgbs"]), p(a["grad_all"]), p(a["grad_omega"]), p(a["grad_or"]), p(a["grad_view_dep"]), p(a["grad_diffuse"]),
                                p(a["grad_clip_feat"]), p(a["grad_smooth_norm"]), p(a["grad_basis_color"]), p(a["ws"]), u64(nbytes)), arrays,
                  f"pnr_palette_train_shade_backward M={M} nb={nb} clip={clip_dim} optional={optional}")


@guards("pnr_palette_smooth_points", "pnr_palette_smooth_forward", "pnr_palette_smooth_backward")
@pytest.mark.parametrize("clip_dim", PAL_CLIPS)
@pytest.mark.parametrize("nb", PAL_BASES)
def test_palette_smooth(cuda, nb, clip_dim):
    bound = 2.0
    for M in PAL_ROWS:
        xyzs = uni(1, M, 3, lo=-2.1, hi=2.1)
        if (nb, clip_dim) == (PAL_BASES[0], PAL_CLIPS[0]):
            # a 16-byte-aligned start (the float4 path; floor(3 M / 4) groups and an element-wise rest) and an element-aligned one (element-wise)
            arrays = dict(xyzs=I(xyzs), noise=I(uni(2, M, 3)), xyzs_diff=O(empty(M, 3)))
            ref, _ = check(lambda a: abi("pnr_palette_smooth_points", p(a["xyzs"]), p(a["noise"]), bound, M, p(a["xyzs_diff"])), arrays,
                           f"pnr_palette_smooth_points M={M}", modes=("aligned", 16, 4))
            assert torch.equal(ref["xyzs_diff"], torch.clamp(xyzs + uni(2, M, 3) * bound * 0.03, -bound, bound))       # the torch expression, bit for bit
        clip = lambda seed: I(rnd(seed, M, clip_dim)) if clip_dim else None  # noqa: E731
        pairs = dict(omega=I(uni(5, M, nb)), omega_diff=I(uni(6, M, nb)), clip_feat=clip(7), clip_feat_diff=clip(8))
        arrays = dict(xyzs=I(xyzs), xyzs_diff=I(xyzs + 0.01), diffuse=I(uni(3, M, 3)), diffuse_diff=I(uni(4, M, 3)), **pairs, smooth_weight=O(empty(M)),
                      smooth_norm=O(empty(M)))
        ref, _ = check(lambda a: abi("pnr_palette_smooth_forward", M, nb, clip_dim, p(a["xyzs"]), p(a["xyzs_diff"]), p(a["diffuse"]), p(a["diffuse_diff"]), p(a["omega"]),
                                     p(a["omega_diff"]), p(a["clip_feat"]), p(a["clip_feat_diff"]), bound, 0.005, 0.2, 0.1, p(a["smooth_weight"]), p(a["smooth_norm"])),
                       arrays, f"pnr_palette_smooth_forward M={M} nb={nb} clip={clip_dim}")
        for optional in (True, False):
            both = optional and clip_dim
            arrays = dict(grad_smooth_norm=I(rnd(9, M)), smooth_weight=I(ref["smooth_weight"]), **pairs, grad_omega=O(empty(M, nb)), grad_omega_diff=O(empty(M, nb)),
                          grad_clip_feat=O(empty(M, clip_dim)) if both else None, grad_clip_feat_diff=O(empty(M, clip_dim)) if both else None)
            check(lambda a: abi("pnr_palette_smooth_backward", M, nb, clip_dim, p(a["grad_smooth_norm"]), p(a["smooth_weight"]), p(a["omega"]), p(a["omega_diff"]),
                                p(a["clip_feat"]), p(a["clip_feat_diff"]), p(a["grad_omega"]), p(a["grad_omega_diff"]), p(a["grad_clip_feat"]),
                                p(a["grad_clip_feat_diff"])), arrays, f"pnr_palette_smooth_backward M={M} nb={nb} clip={clip_dim} optional={optional}")


LOSS_POINTERS = ("weights_sum", "depth_raw", "image_raw", "all_map", "nears", "fars", "bg_color", "gt_rgb", "gt_clip", "gt_weights", "basis_color", "basis_color_origin",
                 "image", "depth", "direct_rgb", "loss_ray", "terms", "grad_loss", "grad_weights_sum", "grad_image_raw", "grad_all_map", "grad_basis_color", "workspace")


def loss_args(a, N, nb, clip_dim, bg_mode, nbytes):
    t = _lib.TrainLossArgs()
    palette = a.get("all_map") is not None
    t.N, t.n_channel, t.num_basis, t.clip_dim = N, (13 + clip_dim + nb) if palette else 0, nb if palette else 0, clip_dim if palette else 0
    t.bg_const, t.bg_mode = 1.0, bg_mode
    t.lambda_sparsity, t.lambda_offsets, t.lambda_view_dep, t.lambda_smooth, t.lambda_weight, t.lambda_palette = 2e-4, 0.03, 0.1, 4e-3, 0.05, 1e-3
    for name in LOSS_POINTERS:
        setattr(t, name, p(a.get(name)))
    t.workspace_bytes = nbytes
    return t


@guards("pnr_train_loss_forward", "pnr_train_loss_backward", "pnr_train_loss_backward_bg")
@pytest.mark.parametrize("bg_mode", [0, 1, 2])
@pytest.mark.parametrize("nb,clip_dim", [(0, 0), (1, 0), (4, 16), (10, 32)])       # nb 0: the NeRF model's loss (no all_map)
def test_train_loss(cuda, nb, clip_dim, bg_mode):
    palette = nb > 0
    n_channel = 13 + clip_dim + nb
    for N in PAL_ROWS:
        nbytes = nbytes_of("pnr_train_loss_workspace_bytes", N)
        ins = dict(weights_sum=I(uni(1, N)), depth_raw=I(uni(2, N, hi=4.0)), image_raw=I(uni(3, N, 3)), all_map=I(uni(4, N, n_channel)) if palette else None,
                   nears=I(uni(5, N, lo=0.2, hi=0.5)), fars=I(uni(6, N, lo=3.0, hi=5.0)), bg_color=[None, I(uni(7, 3)), I(uni(7, N, 3))][bg_mode], gt_rgb=I(uni(8, N, 3)),
                   gt_clip=I(rnd(9, N, clip_dim)) if palette and clip_dim else None, gt_weights=I(uni(10, N, nb)) if palette else None,
                   basis_color=I(uni(11, nb, 3)) if palette else None, basis_color_origin=I(uni(12, nb, 3)) if palette else None)
        what = f"N={N} nb={nb} clip={clip_dim} bg_mode={bg_mode}"
        arrays = dict(**ins, image=O(empty(N, 3)), depth=O(empty(N)), direct_rgb=O(empty(N, 3)) if palette else None, loss_ray=O(empty(N)), terms=O(empty(10)),
                      workspace=WS(nbytes, zero=True))
        check(lambda a: abi("pnr_train_loss_forward", ctypes.byref(loss_args(a, N, nb, clip_dim, bg_mode, nbytes))), arrays, "pnr_train_loss_forward " + what)
        ins["grad_loss"] = I(torch.full((1,), 0.75, device="cuda"))
        arrays = dict(**ins, grad_weights_sum=O(empty(N)), grad_image_raw=O(empty(N, 3)), grad_all_map=O(empty(N, n_channel)) if palette else None,
                      grad_basis_color=O(empty(nb, 3)) if palette else None)
        check(lambda a: abi("pnr_train_loss_backward", ctypes.byref(loss_args(a, N, nb, clip_dim, bg_mode, 0))), arrays, "pnr_train_loss_backward " + what)
        if bg_mode == 2:
            arrays = dict(**ins, grad_bg_color=O(empty(N, 3)))
            check(lambda a: abi("pnr_train_loss_backward_bg", ctypes.byref(loss_args(a, N, nb, clip_dim, bg_mode, 0)), p(a["grad_bg_color"])), arrays,
                  "pnr_train_loss_backward_bg " + what)


# ================================================================ fused fields (32-sample wave tiles, 128-row workgroups) and the background model
FIELD_ROWS = (1, 127, 129)
NERF_SHAPES = ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))        # sigma0, sigma1, color0, color1, color2


@functools.lru_cache(maxsize=None)
def nerf_blob(precision):
    ws = [rnd(10 + k, *shape, scale=0.3) for k, shape in enumerate(NERF_SHAPES)]
    blob = torch.zeros(nbytes_of("pnr_nerf_field_packed_bytes"), dtype=torch.uint8, device="cuda")
    assert abi("pnr_nerf_field_pack", *[p(w) for w in ws], p(blob), precision) == 0
    torch.cuda.synchronize()
    return ws, blob


@guards("pnr_nerf_field_pack", "pnr_nerf_field_forward", "pnr_nerf_density_forward")
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_nerf_field(cuda, precision):
    ws, blob = nerf_blob(precision)
    arrays = {f"w{k}": I(w) for k, w in enumerate(ws)}
    arrays["packed"] = O(torch.zeros_like(blob), weak=16)           # exactly pnr_nerf_field_packed_bytes
    ref, _ = check(lambda a: abi("pnr_nerf_field_pack", *[p(a[f"w{k}"]) for k in range(5)], p(a["packed"]), precision), arrays, f"pnr_nerf_field_pack {precision}")
    assert same_bits(ref["packed"], blob)
    for B in FIELD_ROWS:
        enc, dirs = rnd(B, 16, B, 2, scale=0.1), unit_dirs(B + 1, B)
        for enc_scale in (1.0, 64.0):
            arrays = dict(enc=I(enc), dirs=I(dirs), packed=I(blob, around=0xFF, weak=16), sigmas=O(empty(B)), rgbs=O(empty(B, 3)))
            check(lambda a: abi("pnr_nerf_field_forward", p(a["enc"]), p(a["dirs"]), p(a["packed"]), B, p(a["sigmas"]), p(a["rgbs"]), precision, enc_scale), arrays,
                  f"pnr_nerf_field_forward B={B} precision={precision} enc_scale={enc_scale}")
        for geo in (True, False):
            arrays = dict(enc=I(enc), packed=I(blob, around=0xFF, weak=16), sigmas=O(empty(B)), geo_feat=O(empty(B, 15)) if geo else None)
            check(lambda a: abi("pnr_nerf_density_forward", p(a["enc"]), p(a["packed"]), B, 0.5, p(a["sigmas"]), p(a["geo_feat"]), precision, 1.0), arrays,
                  f"pnr_nerf_density_forward B={B} precision={precision} geo={geo}")


PALETTE_WEIGHTS = dict(sigma0=(64, 32), sigma1=(16, 64), diff0=(64, 15), diff1=(64, 64), diff2=(3, 64), color0=(64, 31), color1=(64, 64), color2=(3, 64), basis0=(64, 35),
                       basis1=(15, 64))


def palette_weight_tensors(nb, clip_dim, pred_clip):
    shapes = dict(PALETTE_WEIGHTS, offsets_radiance=(3 * nb + 1, 15), omega=(nb, 15), basis_color=(nb, 3), or_bias=(3 * nb + 1,))
    if pred_clip:
        shapes.update(clip0=(64, 32), clip1=(clip_dim, 64))
    return {name: rnd(20 + k, *shape, scale=0.3) for k, (name, shape) in enumerate(shapes.items())}


def palette_pack(a, names, nb, clip_dim, pred_clip, precision):
    pw = _lib.PaletteWeights()
    for name in names:
        setattr(pw, name, p(a[name]))
    pw.num_basis, pw.clip_dim, pw.pred_clip, pw.precision = nb, clip_dim, int(pred_clip), precision
    return abi("pnr_palette_field_pack", ctypes.byref(pw), p(a["packed"]))


@guards("pnr_palette_field_pack", "pnr_palette_field_forward")
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("nb,clip_dim,pred_clip", [(4, 0, False), (8, 16, True), (10, 32, True), (1, 0, False)])
def test_palette_field(cuda, nb, clip_dim, pred_clip, precision):
    lib = _lib.load()
    ws = palette_weight_tensors(nb, clip_dim, pred_clip)
    nbytes = int(lib.pnr_palette_field_packed_bytes(nb, clip_dim, int(pred_clip)))
    aux_stride = int(lib.pnr_palette_aux_channels(nb, clip_dim))
    pack_precision = 1 if precision == 2 else precision           # "same packed blobs" (PNR_FIELD_F16X2)
    arrays = {name: I(w) for name, w in ws.items()}
    arrays["packed"] = O(torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), weak=16)        # exactly pnr_palette_field_packed_bytes
    ref, _ = check(lambda a: palette_pack(a, list(ws), nb, clip_dim, pred_clip, pack_precision), arrays, f"pnr_palette_field_pack nb={nb} clip={clip_dim} {precision}")
    blob = ref["packed"]
    for B in FIELD_ROWS:
        for deltas in (False, True):
            dl = uni(B, B, 2, lo=0.001, hi=0.01)
            dl[::3, 0] = 0                                        # rows with deltas[:, 0] == 0 are skipped
            arrays = dict(enc=I(rnd(B, 16, B, 2, scale=0.1)), enc_palette=I(rnd(B + 1, 16, B, 2, scale=0.1)), enc_clip=I(rnd(B + 2, 16, B, 2, scale=0.1)) if pred_clip else None,
                          dirs=I(unit_dirs(B + 3, B)), deltas=I(dl) if deltas else None, packed=I(blob, around=0xFF, weak=16), sigmas=O(empty(B)), rgbs=O(empty(B, 3)),
                          aux=O(empty(B, aux_stride)))

            def call(a):
                t = _lib.PaletteFieldArgs()
                t.B, t.level_stride, t.num_basis, t.clip_dim, t.pred_clip, t.aux_stride, t.precision = B, B, nb, clip_dim, int(pred_clip), aux_stride, precision
                t.density_scale, t.offsets_weight, t.view_dep_weight = 1.0, 1.0, 1.0
                for name in ("enc", "enc_palette", "enc_clip", "dirs", "deltas", "packed", "sigmas", "rgbs", "aux"):
                    setattr(t, name, p(a[name]))
                return abi("pnr_palette_field_forward", ctypes.byref(t))

            check(call, arrays, f"pnr_palette_field_forward B={B} nb={nb} clip={clip_dim} precision={precision} deltas={deltas}")


BG = dict(D=2, C=2, L=4, H=16, pls=float(np.exp2(np.log2(2048 / 16) / 3)), log2T=19)     # encoder_bg of both networks


def background_common(t, a, N, rows):
    t.N, t.rays_o, t.rays_d, t.radius, t.coords_in = N, p(a.get("rays_o")), p(a["rays_d"]), 4.0, p(a.get("coords_in"))
    t.embeddings, t.offsets, t.table_rows = p(a["embeddings"]), p(a["offsets"]), rows
    t.num_levels, t.level_dim, t.S, t.H, t.gridtype, t.align_corners = 4, 2, float(np.log2(BG["pls"])), 16, 0, 0
    t.sh_degree, t.num_layers, t.hidden_dim = 4, 2, 64
    return t


@guards("pnr_background_pack", "pnr_background_forward", "pnr_background_train_forward", "pnr_background_backward")
@pytest.mark.parametrize("N", FIELD_ROWS)
def test_background(cuda, N):
    from tests.test_gpu_background import rays_outside_in
    from tests.test_gpu_background_train import BOUND as GRAD_BOUND
    offsets = grid_offsets(BG, False)
    rows = int(offsets[-1])
    table, w0, w1 = (uni(1, rows, 2) - 0.5) * 0.5, rnd(2, 64, 24, scale=0.3), rnd(3, 3, 64, scale=0.3)
    o, d = rays_outside_in(cuda, N, seed=N)
    off = I(dev(offsets), around=(rows,))
    nbytes = nbytes_of("pnr_background_packed_bytes")
    arrays = dict(w0=I(w0), w1=I(w1), packed=O(torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), weak=16))
    blob = check(lambda a: abi("pnr_background_pack", p(a["w0"]), p(a["w1"]), p(a["packed"])), arrays, "pnr_background_pack")[0]["packed"]
    for dtype in (0, 1):
        for with_coords in (False, True):
            arrays = dict(rays_o=I(o), rays_d=I(d), embeddings=I(table.to(DT[dtype]), weak=8 >> dtype), offsets=off, packed=I(blob, around=0xFF, weak=16), out=O(empty(N, 3)),
                          coords_out=O(empty(N, 2), weak=8) if with_coords else None)

            def fwd(a):
                t = background_common(_lib.BackgroundArgs(), a, N, rows)
                t.table_dtype, t.packed, t.out, t.coords_out = dtype, p(a["packed"]), p(a["out"]), p(a["coords_out"])
                return abi("pnr_background_forward", ctypes.byref(t))

            check(fwd, arrays, f"pnr_background_forward N={N} dtype={dtype} coords_out={with_coords}")
            if with_coords:     # float2 accesses of the coordinates, 8- / 4-byte rows of the table: a start 4 bytes off an 8-byte boundary is refused, nothing is written
                check(fwd, arrays, f"pnr_background_forward misaligned N={N} dtype={dtype}", expect=ERR_ALIGNMENT, modes=(4,))
    arrays = dict(rays_o=I(o), rays_d=I(d), embeddings=I(table, weak=8), offsets=off, w0=I(w0), w1=I(w1), out=O(empty(N, 3)), coords_out=O(empty(N, 2), weak=8))

    def train_fwd(a):
        t = background_common(_lib.BackgroundTrainArgs(), a, N, rows)
        t.w0, t.w1, t.out, t.coords_out = p(a["w0"]), p(a["w1"]), p(a["out"]), p(a["coords_out"])
        return abi("pnr_background_train_forward", ctypes.byref(t))

    ref, _ = check(train_fwd, arrays, f"pnr_background_train_forward N={N}")
    nb = nbytes_of("pnr_background_backward_workspace_bytes", N)

    # float atomics: each call's grad_table is held to the float64 gradient as tests/test_gpu_background_train.py holds it -- within BOUND of the reference's
    # largest entry -- and the rows no ray reaches stay exactly zero
    from oracle.torch_encoders import TorchSHEncoder
    grad_rgb = rnd(4, N, 3)
    x01 = ((ref["coords_out"].cpu().numpy() + np.float32(1)) / np.float32(2)).astype(np.float32)
    G = gr.GridReference(x01, offsets, BG["pls"], BG["H"], 0, False)
    feat = torch.from_numpy(G.forward(table.cpu().numpy())[0].reshape(N, -1)).requires_grad_(True)
    h = torch.cat([TorchSHEncoder(degree=4)(d.double().cpu()), feat], dim=-1)
    rgb = torch.sigmoid(torch.relu(h @ w0.double().cpu().T) @ w1.double().cpu().T)
    (rgb * grad_rgb.double().cpu()).sum().backward()
    want, _, addends = G.table_grad(feat.grad.numpy())
    reached = torch.from_numpy(addends > 0).cuda()

    def close(got, plain):
        for name, t in (("guarded", got), ("plain", plain)):
            assert nans(t) == 0
            err = float(np.abs(t.double().cpu().numpy() - want).max())
            assert err <= GRAD_BOUND * float(np.abs(want).max()), f"grad_table ({name} call): {err} against the float64 gradient"
            assert not bool(t[~reached].any()), f"grad_table ({name} call): a row no ray reaches was written"

    arrays = dict(rays_d=I(d), coords_in=I(ref["coords_out"], weak=8), embeddings=I(table, weak=8), offsets=off, w0=I(w0), w1=I(w1), grad_rgb=I(grad_rgb),
                  grad_w0=O(empty(64, 24)), grad_w1=O(empty(3, 64)), grad_table=O(torch.zeros(rows, 2, device="cuda")), ws=WS(nb, weak=16))

    def bwd(a):
        t = background_common(_lib.BackgroundTrainArgs(), a, N, rows)
        t.w0, t.w1, t.grad_rgb, t.grad_w0, t.grad_w1, t.grad_table = p(a["w0"]), p(a["w1"]), p(a["grad_rgb"]), p(a["grad_w0"]), p(a["grad_w1"]), p(a["grad_table"])
        t.workspace, t.workspace_bytes = p(a["ws"]), nb
        return abi("pnr_background_backward", ctypes.byref(t))

    check(bwd, arrays, f"pnr_background_backward N={N}", close={"grad_table": close})


# ================================================================ the frame loops, one-call form
@functools.lru_cache(maxsize=None)
def frame_model(kind):
    """nerf; palette4 (4 bases, no clip head: the pair table); palette8 (8 bases and a clip head: the triple table).  Scene S0, seeded weights."""
    from palettenerf_amd import fused, network, raymarching, renderer, scene
    if kind == "nerf":
        m = network.NeRFNetwork(bound=2, cuda_ray=True, min_near=0.2)
    else:
        opt = renderer.default_opt() if kind == "palette4" else renderer.default_opt(num_basis=8, pred_clip=True)
        m = network.PaletteNetwork(opt, bound=2, cuda_ray=True, min_near=0.2)
    scene.seed_field_(m, 3)
    m = m.cuda().eval()
    m.density_grid.copy_(scene_s0()["grid"])
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m, (fused.NeRFFieldFused(m) if kind == "nerf" else fused.PaletteFieldFused(m))


def frame_rays(N):
    """N rays of a 40 x 40 frame of S0, the centre first"""
    from palettenerf_amd import scene
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(40, 40), 40, 40)
    yy, xx = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    ids = torch.from_numpy(np.argsort(np.maximum(np.abs(yy - 19.5), np.abs(xx - 19.5)).reshape(-1), kind="stable")[:N])
    return ro[0][ids].contiguous().cuda(), rd[0][ids].contiguous().cuda()


@guards("pnr_nerf_render_frame", "pnr_palette_render_frame", "pnr_interleave_tables", "pnr_interleave_tables3", "pnr_interleave_tables3_half")
@pytest.mark.parametrize("N", [1, 257, 1600])
@pytest.mark.parametrize("kind", ["nerf", "palette4", "palette8"])
def test_render_frame(cuda, kind, N):
    m, f = frame_model(kind)
    lib = _lib.load()
    ro, rd = frame_rays(N)
    aabb = m.aabb_infer.detach().float().contiguous()
    # the project's own preparation fills the argument struct (settings, precision, tables, blob); the calls below run on copies of it with their own arrays
    tok = f.frame_prepare(ro, rd, None, None, 0.0, 1024, 1e-4, bg_color=1.0, aabb=aabb, min_near=m.min_near)
    args, base = tok.args, tok.base
    palette = kind != "nerf"
    if palette:
        nbytes = int(lib.pnr_palette_frame_workspace_bytes(N, f.nb, f.clip_dim, int(f.pred_clip)))
        assert (f.nb, bool(f.pred_clip)) == ((4, False) if kind == "palette4" else (8, True))
    else:
        nbytes = int(lib.pnr_nerf_frame_workspace_bytes(N))
    assert base.workspace_bytes == nbytes and base.aabb and base.finish        # exactly *_frame_workspace_bytes; near / far computed by the call; the epilogue applied
    enc = m.encoder
    rows = enc.embeddings.shape[0]
    mip, blob = tok.keep[0], tok.keep[2]
    arrays = dict(rays_o=I(ro), rays_d=I(rd), nears=O(empty(N)), fars=O(empty(N)), bitfield=I(m.density_bitfield, around=0x00, weak=8),
                  mip=I(mip.view(-1).view(torch.uint8), around=0x00, weak=8), embeddings=I(enc.embeddings.detach()), offsets=I(enc.offsets, around=(rows,)),
                  packed_weights=I(blob.view(-1).view(torch.uint8), around=0xFF, weak=16), weights_sum=O(empty(N)), depth=O(empty(N)), image=O(empty(N, 3)),
                  workspace=WS(nbytes), aabb=I(aabb), depth_raw=O(empty(N)) if base.depth_raw else None)
    outer = {}
    if palette:
        outer = dict(embeddings_palette=I(m.encoder_palette.embeddings.detach()), aux_map=O(empty(N, f.aux_channels)))
        if f.pred_clip:
            outer["embeddings_clip"] = I(m.encoder_clip.embeddings.detach())
            triple = f._triple_table()
            outer["embeddings_triple"] = I(triple, weak=32)         # one 32-byte row per corner
            ts = [e.embeddings.detach() for e in (m.encoder, m.encoder_palette, m.encoder_clip)]
            t_arrays = dict(a=I(ts[0]), b=I(ts[1]), c=I(ts[2]), out=O(torch.zeros_like(triple), weak=32))
            ref, _ = check(lambda a: abi("pnr_interleave_tables3", p(a["a"]), p(a["b"]), p(a["c"]), u64(rows), p(a["out"])), t_arrays, "pnr_interleave_tables3")
            assert same_bits(ref["out"], triple)
            if N == 1:      # the fp16 form of the same rows (the -O frames' table), once
                t_arrays["out"] = O(torch.zeros(rows, 8, dtype=torch.float16, device="cuda"), weak=16)
                ref, _ = check(lambda a: abi("pnr_interleave_tables3_half", p(a["a"]), p(a["b"]), p(a["c"]), u64(rows), p(a["out"])), t_arrays,
                               "pnr_interleave_tables3_half")
                assert torch.equal(ref["out"][:, :6], torch.cat(ts, dim=1).to(torch.float16)) and not bool(ref["out"][:, 6:].any())
        else:
            pair = f._pair_table()
            outer["embeddings_pair"] = I(pair, weak=16)
            t_arrays = dict(a=I(enc.embeddings.detach()), b=I(m.encoder_palette.embeddings.detach()), out=O(torch.zeros_like(pair), weak=16))
            ref, _ = check(lambda a: abi("pnr_interleave_tables", p(a["a"]), p(a["b"]), u64(rows), p(a["out"])), t_arrays, "pnr_interleave_tables")
            assert same_bits(ref["out"], pair)
        for name in ("embeddings_palette", "embeddings_clip", "embeddings_pair", "embeddings_triple", "aux_map"):
            assert bool(getattr(args, name)) == (name in outer), name       # every device pointer of the struct is one of the guarded arrays
    for name, kind_ in _lib.NerfFrameArgs._fields_:
        if kind_ is ctypes.c_void_p and name not in ("stats", "kernel_ms"):
            assert bool(getattr(base, name)) == (arrays.get(name) is not None), name
    arrays.update(outer)

    def call(a):
        mine = type(args).from_buffer_copy(args)
        b = mine.base if palette else mine
        for name in arrays:
            setattr(mine if name in outer else b, name, p(a[name]))
        stats = (ctypes.c_uint64 * 6)()
        b.stats, b.kernel_ms = ctypes.cast(stats, ctypes.c_void_p), None
        rc = abi(f._frame_entry, ctypes.byref(mine))
        torch.cuda.synchronize()
        assert rc != 0 or (stats[0] > 0 and stats[5] == 0), list(stats)
        return rc

    ref, _ = check(call, arrays, f"{f._frame_entry} {kind} N={N}")
    assert float(ref["weights_sum"].max()) > 0.5 or N == 1        # the rays see the scene
