"""Float64 statement of the multiresolution grid encoder for any D, C, gridtype and align_corners, with the error bounds the tests hold the oracle and
the HIP kernels to.  TEST HELPER (imported by tests/test_oracle.py and tests/test_gpu_grid_variants.py); numpy only, no GPU.

What is shared with the code under test are the kernels' INPUTS only: the per-level (scale, resolution) of oracle.grid_level_params and the fp32 cell
position (one rounding of x * scale [+ 0.5], its floor, the fp32 fractional part).  Everything after that -- corner weights, sums, differences, scatter --
is float64 here, so a result of this module is the exact value up to ~2^-53 and every bound below is a bound on the fp32 / fp16 arithmetic of the code
under test alone.  The row index is integer arithmetic modulo 2^32 (uint64 values masked after every step), as grid_core.hpp:grid_index does it.

Bounds (u = 2^-24 for an fp32 table, 2^-11 for an fp16 one; S = the sum of the absolute values of the float64 terms of the element):
  forward          (2^D + D + 3) u S          2^D fused multiply-adds, D + 3 for the roundings inside a corner weight
  dy_dx            (2^(D-1) + D + 3) u S      the same with 2^(D-1) (right - left) terms, the weight includes `scale`
  table gradient   (n + D + 3) u S            n addends reach the row, in any order (atomics, the segmented wave sum, a loop: all covered)
  input gradient   (L C + D + 3) u S          S = sum |g| * (sum |w (right - left)|): the terms behind each dy_dx count one by one
fp16 tables add an absolute term for roundings that end in half's subnormal range (spacing 2^-24): one per addend.
The fp16 forward bound is derived from the two roundings per corner of the half accumulator, acc = half(float(acc) + float(half(w * e))): the product
rounds once (u |w e|, or 2^-25 absolute when subnormal), the sum rounds once (u |partial sum| <= u S): (2^D + 1) u S + 2^D 2^-25, stated with the same
D + 3 slack for the weight and twice the absolute term.
"""
import functools

import numpy as np

import oracle

PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037)   # grid_core.hpp:grid_index, one per dimension
_MASK = np.uint64(0xFFFFFFFF)
U32, U16 = 2.0 ** -24, 2.0 ** -11
HALF_TINY = 2.0 ** -24                                          # spacing of fp16 subnormals


class GridReference:
    """Cells, rows and weights of `x` [B, D] float32 on every level (independent of the table), then float64 forward / dy_dx / gradients for a table."""

    def __init__(self, x, offsets, per_level_scale, base_resolution, gridtype=0, align_corners=False):
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 2
        offsets = np.asarray(offsets).astype(np.int64)
        self.B, self.D = x.shape
        self.L, self.rows_total = len(offsets) - 1, int(offsets[-1])
        B, D, L = self.B, self.D, self.L
        scale, res = oracle.grid_level_params(L, per_level_scale, base_resolution)
        self.scale = scale.astype(np.float64)
        self.inr = ((x >= 0) & (x <= 1)).all(axis=1)             # exactly 0.0 and 1.0 are inside
        xs = np.where(self.inr[:, None], x, np.float32(0)).astype(np.float64)
        self.f = np.empty((L, D, 2, B))                          # factor of dimension d when the corner's bit d is 0 / 1
        self.rows = np.empty((L, 1 << D, B), np.int64)           # table row (level offset included) of every corner
        for l in range(L):
            # the product of two binary32 numbers is exact in binary64: one rounding to fp32, as fmaf gives
            pos = (xs * np.float64(scale[l]) + (0.0 if align_corners else 0.5)).astype(np.float32)
            pg = np.floor(pos)
            fr = (pos - pg).astype(np.float32).astype(np.float64)
            self.f[l, :, 0], self.f[l, :, 1] = (1.0 - fr).T, fr.T
            size = int(offsets[l + 1] - offsets[l])
            side = int(res[l]) if align_corners else int(res[l]) + 1
            pgu = pg.astype(np.uint64)
            for corner in range(1 << D):
                c = [(pgu[:, d] + np.uint64((corner >> d) & 1)) & _MASK for d in range(D)]
                stride, index = 1, np.zeros(B, np.uint64)
                for d in range(D):
                    if stride <= size:
                        index = (index + c[d] * np.uint64(stride)) & _MASK
                        stride = (stride * side) & 0xFFFFFFFF
                if gridtype == 0 and stride > size:
                    index = np.zeros(B, np.uint64)
                    for d in range(D):
                        index ^= (c[d] * np.uint64(PRIMES[d])) & _MASK
                self.rows[l, corner] = (index % np.uint64(size)).astype(np.int64) + offsets[l]

    def _weights(self, l, corners, skip=None):
        """[len(corners), B]: product over the dimensions (but `skip`) of the factor each corner's bit selects"""
        w = np.ones((len(corners), self.B))
        for d in range(self.D):
            if d != skip:
                w = w * self.f[l, d][(corners >> d) & 1]
        return w

    def forward(self, table):
        """-> (out [B, L, C], sum |w e| [B, L, C])"""
        table = np.asarray(table, np.float64)
        out = np.zeros((self.B, self.L, table.shape[1]))
        mag = np.zeros_like(out)
        corners = np.arange(1 << self.D)
        for l in range(self.L):
            t = self._weights(l, corners)[:, :, None] * table[self.rows[l]]
            out[:, l], mag[:, l] = t.sum(axis=0), np.abs(t).sum(axis=0)
        out[~self.inr], mag[~self.inr] = 0, 0
        return out, mag

    def dy_dx(self, table):
        """-> (d out / d x [B, L, D, C], sum |w (right - left)| [B, L, D, C]); w includes the level's scale"""
        table = np.asarray(table, np.float64)
        dy = np.zeros((self.B, self.L, self.D, table.shape[1]))
        mag = np.zeros_like(dy)
        corners = np.arange(1 << self.D)
        for l in range(self.L):
            for gd in range(self.D):
                left = corners[(corners >> gd) & 1 == 0]
                w = self.scale[l] * self._weights(l, left, skip=gd)
                t = w[:, :, None] * (table[self.rows[l, left | (1 << gd)]] - table[self.rows[l, left]])
                dy[:, l, gd], mag[:, l, gd] = t.sum(axis=0), np.abs(t).sum(axis=0)
        dy[~self.inr], mag[~self.inr] = 0, 0
        return dy, mag

    def table_grad(self, grad):
        """grad [B, L*C] -> (d / d table [rows, C], sum |w g| [rows, C], number of addends per row [rows])"""
        g = np.asarray(grad, np.float64).reshape(self.B, self.L, -1)
        C = g.shape[2]
        gt = np.zeros((self.rows_total, C))
        mag = np.zeros_like(gt)
        n = np.zeros(self.rows_total, np.int64)
        sel = self.inr                                           # out-of-range samples scatter nothing
        corners = np.arange(1 << self.D)
        for l in range(self.L):
            rows = self.rows[l][:, sel].reshape(-1)
            t = (self._weights(l, corners)[:, sel, None] * g[sel, l][None]).reshape(-1, C)
            n += np.bincount(rows, minlength=self.rows_total)
            for ch in range(C):
                gt[:, ch] += np.bincount(rows, weights=t[:, ch], minlength=self.rows_total)
                mag[:, ch] += np.bincount(rows, weights=np.abs(t[:, ch]), minlength=self.rows_total)
        return gt, mag, n

    def input_grad(self, grad, dy, dy_mag):
        """grad [B, L*C], (dy, dy_mag) of dy_dx() -> (d / d x [B, D], sum |g| sum |w (right - left)| [B, D])"""
        g = np.asarray(grad, np.float64).reshape(self.B, self.L, 1, -1)
        return (g * dy).sum(axis=(1, 3)), (np.abs(g) * dy_mag).sum(axis=(1, 3))


def forward_bound(D, mag, u=U32):
    return (2 ** D + D + 3) * u * mag + (0 if u == U32 else 2 ** D * HALF_TINY)


def dy_dx_bound(D, mag):
    return (2 ** (D - 1) + D + 3) * U32 * mag


def table_grad_bound(D, mag, n, u=U32):
    return (n[:, None] + D + 3) * u * mag + (0 if u == U32 else n[:, None] * HALF_TINY)


def input_grad_bound(D, L, C, mag, u=U32):
    return (L * C + D + 3) * u * mag


def error_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 the value has to be exact (else inf).  NaN if `got` holds one."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    zero = bound == 0
    if np.isnan(err).any():
        return float("nan")
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ------------------------------------------------------------------------------------------ the variant matrix's cases
# L = 6, H = 16, per_level_scale = 2: scales 15 ... 511, so levels 0-4 take the run-combining backward kernel (scale <= 384) and level 5 the plain one
L, H, PLS = 6, 16, 2.0
EXTRA_LOG2T = {1: 3, 2: 6}      # with 2^10 rows most levels of a D <= 2 grid are dense: a second, tiny table so that hashed levels occur as well
ODD_SIZES = (13, 29, 61, 101, 251, 509)   # rows per level: hashed for every D (below the level's side), no power of two, no multiple of 8; even total


def variant_cases(D):
    """[(name, offsets, gridtype, align_corners)]: gridtype x align_corners on the encoder's own offsets, plus hand-made odd level sizes (hash)."""
    cases = []
    for log2T in [10] + ([EXTRA_LOG2T[D]] if D in EXTRA_LOG2T else []):
        for gridtype in (0, 1):
            for ac in (False, True):
                name = f"T{log2T}-{'tiled' if gridtype else 'hash'}{'-ac' if ac else ''}"
                cases.append((name, oracle.grid_offsets(D, L, PLS, H, log2T, align_corners=ac), gridtype, ac))
    cases.append(("odd-sizes-hash", np.concatenate([[0], np.cumsum(ODD_SIZES)]).astype(np.int32), 0, False))
    return cases


@functools.lru_cache(maxsize=None)
def variant_inputs(D):
    """{"rays": [999, D], "uniform": [257, D]} float32.  rays: 37 segments of 27 consecutive samples that advance by a constant step of ~0.1 / 27, so on
    the coarse levels consecutive samples share a cell (runs of 2-27 equal rows that start and end anywhere in a 64-lane wave, across wave and block
    edges and in the ragged last wave), with out-of-range samples inside runs, a block of identical rows and the boundary values.  uniform: runs of 1."""
    rng = np.random.default_rng(1000 + D)
    start = rng.random((37, 1, D)) * 0.9
    step = (0.1 / 27) * (0.5 + 0.5 * rng.random((37, 1, D)))
    x = (start + np.arange(27)[None, :, None] * step).reshape(999, D).astype(np.float32)
    assert x.min() >= 0 and x.max() < 1
    x[100] = 1.0e6                      # far outside, in the middle of segment 3
    x[200, D - 1] = -0.25               # one negative coordinate
    x[300:310] = x[300]                 # ten identical rows
    x[400] = 0.0
    x[401] = 1.0                        # align_corners: the +1 corner sits at index `side`, beyond a dense level -- the `%` wraps it
    x[500, 0] = 1.0000001               # one ulp above 1: outside
    x[600, D // 2] = -1e-7              # just below 0: outside
    return {"rays": x, "uniform": rng.random((257, D)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def variant_geometry(D, case_index, input_name):
    _, offsets, gridtype, ac = variant_cases(D)[case_index]
    return GridReference(variant_inputs(D)[input_name], offsets, PLS, H, gridtype, ac)


def variant_tables(D, C, case_index):
    """(fp32 table, output gradient for 999 rows [999, L*C] fp32 standard normal) of one case; deterministic"""
    rng = np.random.default_rng(5000 + 100 * D + 10 * C + case_index)
    rows = int(variant_cases(D)[case_index][1][-1])
    return (rng.random((rows, C)) - 0.5).astype(np.float32), rng.standard_normal((999, L * C)).astype(np.float32)
