"""Float64 statement of the multiresolution grid encoder for any D, C, gridtype and align_corners, with the error bounds the tests hold the oracle and
the HIP kernels to.  TEST HELPER (imported by tests/test_oracle.py, tests/test_gpu_grid_variants.py, tests/test_gpu_grid_binned.py and tests/test_gpu_reference_grid.py); numpy only, no GPU.

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

    def table_grad_sparse(self, grad):
        """table_grad() restricted to the rows a sample reaches -> (touched rows [T] ascending, d / d table [T, C], sum |w g| [T, C], addends [T]).  For
        tables of millions of rows of which a batch touches few: the same addends summed in the same order (np.bincount adds in input order), so the
        values are those of table_grad() bit for bit (tests/test_oracle.py shows it on a variant case)."""
        g = np.asarray(grad, np.float64).reshape(self.B, self.L, -1)
        C = g.shape[2]
        sel = self.inr
        touched, compact = np.unique(self.rows[:, :, sel], return_inverse=True)
        compact = compact.reshape(self.L, 1 << self.D, -1)
        T = len(touched)
        gt, mag, n = np.zeros((T, C)), np.zeros((T, C)), np.zeros(T, np.int64)
        corners = np.arange(1 << self.D)
        for l in range(self.L):
            rows = compact[l].reshape(-1)
            t = (self._weights(l, corners)[:, sel, None] * g[sel, l][None]).reshape(-1, C)
            n += np.bincount(rows, minlength=T)
            for ch in range(C):
                gt[:, ch] += np.bincount(rows, weights=t[:, ch], minlength=T)
                mag[:, ch] += np.bincount(rows, weights=np.abs(t[:, ch]), minlength=T)
        return touched, gt, mag, n

    def table_grad_from_sparse(self, grad):
        """table_grad()'s dense triple, assembled from table_grad_sparse()"""
        touched, s_gt, s_mag, s_n = self.table_grad_sparse(grad)
        gt, n = np.zeros((self.rows_total, s_gt.shape[1])), np.zeros(self.rows_total, np.int64)
        mag = np.zeros_like(gt)
        gt[touched], mag[touched], n[touched] = s_gt, s_mag, s_n
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


# ------------------------------------------------------------------------------------------ the binned table gradient's cases
# csrc/grid_binned.hip (D = 3, C = 2, fp32 tables): the table in buckets of BIN_ROWS rows, gather jobs of at most BIN_CHUNK records, and per level one
# of four treatments chosen by the host (binned_level_plan).  tests/test_gpu_grid_binned.py holds every one of them to table_grad_bound.
#
# No regime needs a bound of its own.  Per addend: D subtractions and D - 1 products for the weight, one product with the gradient = D + 3 roundings,
# then the sum of the n addends of a row --
#   records (COMBINE 0): the values are summed in fp64 (LDS), ONE rounding to fp32; a bucket split into j jobs adds j fp32 partials (the first onto an
#     exact 0): 1 + (j - 1) roundings, and every partial that is not 0 holds at least one addend, so j <= n;
#   merged records (COMBINE 1 / 2): a run of m addends is first summed by a segmented scan of depth ceil(log2 m) <= m - 1 in fp32, then as above;
#   images: each of p <= min(n, workgroups) workgroup partials is rounded to fp32 once (u |partial|, in total <= u S), the reduce adds them in fp32 onto
#     0: the partials that are 0 add exactly, p - 1 roundings remain -- p in all;
# each of them at most n roundings of at most u S: (n + D + 3) u S holds for all.  An entry point that ADDS into a buffer holding p rounds once more:
# u |p + gradient| (table_grad_accumulate_bound).
BIN_ROWS, BIN_CHUNK = 8192, 131072
BINNED_A = (8, 16, 1.5, 17)                                   # L, H, per_level_scale, log2_hashmap_size: scales 15 ... 272.4
BINNED_B_SIZES = (8192, 8193, 16384, 16385, 24577, 70001)     # L = 6, H = 16, per_level_scale = 2; even total
BINNED_CASES = ("A-hash", "A-hash-ac", "A-tiled", "A-tiled-ac", "B-hash", "B-tiled", "C")
BINNED_LONG_RUNS = ((2048, 2064), (3010, 3023))               # lanes 0-15 and 2-14 of a row of 16; these samples stay alive on every level
BINNED_RAYS = 4999                                            # 185 segments of 27 + 4 loose rows: ragged last workgroups at 1024 and 4096 samples each


def binned_case(name):
    """-> (L, H, per_level_scale, offsets, gridtype, align_corners)"""
    gridtype = 1 if "tiled" in name else 0
    if name[0] == "B":
        return 6, 16, 2.0, np.concatenate([[0], np.cumsum(BINNED_B_SIZES)]).astype(np.int32), gridtype, False
    L_, H_, pls, log2T = BINNED_A
    ac = name.endswith("-ac")
    return L_, H_, pls, oracle.grid_offsets(3, L_, pls, H_, log2T, align_corners=ac), gridtype, ac


def binned_level_plan(L_, pls, H_, offsets, align_corners, coarse_image=True, cell_merge=True):
    """The host's choice per level (pnr_grid_encode_backward_binned), recomputed: -> (sizes, buckets, kinds); kinds[l] is "image" (fp64 LDS images, no
    records), 1 (records of runs of equal rows), 2 (records of runs of samples in one cell) or 0 (a record per sample and corner)."""
    scale, res = oracle.grid_level_params(L_, pls, H_)
    sizes = np.diff(np.asarray(offsets).astype(np.int64))
    ni = jobs = 0
    while coarse_image and ni < L_:
        side = int(res[ni]) + (0 if align_corners else 1)
        halves = -(-((side ** 3 + 7) // 8 * 8) // BIN_ROWS)
        if halves > 2 or jobs + halves > 8:
            break
        jobs, ni = jobs + halves, ni + 1
    nc = ni
    while nc < L_ and scale[nc] <= 24.0:
        nc += 1
    nm = nc
    while cell_merge and nm < L_ and scale[nm] <= 256.0:
        nm += 1
    return tuple(int(s) for s in sizes), tuple(int(-(-s // BIN_ROWS)) for s in sizes), ("image",) * ni + (1,) * (nc - ni) + (2,) * (nm - nc) + (0,) * (L_ - nm)


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _binned_rays():
    """[4999, 3] float32, ray-ordered like variant_inputs' "rays" (runs of samples in one cell and of equal rows that start and end anywhere in a wave and
    in a row of 16 lanes), with the same specials inside segments and one block of identical rows across the edge of a 1024-sample workgroup."""
    rng = np.random.default_rng(4999)
    start = rng.random((185, 1, 3)) * 0.9
    step = (0.1 / 27) * (0.5 + 0.5 * rng.random((185, 1, 3)))
    x = np.concatenate([(start + np.arange(27)[None, :, None] * step).reshape(4995, 3), rng.random((4, 3))]).astype(np.float32)
    assert x.shape == (BINNED_RAYS, 3) and x.min() >= 0 and x.max() < 1
    x[100] = 1.0e6                      # far outside, in the middle of segment 3
    x[200, 2] = -0.25                   # one negative coordinate
    x[300:310] = x[300]                 # ten identical rows
    x[400] = 0.0
    x[401] = 1.0
    x[500, 0] = 1.0000001               # one ulp above 1: outside
    x[600, 1] = -1e-7                   # just below 0: outside
    x[1019:1029] = x[1019]              # ten identical rows across a workgroup's (and a wave's) edge
    for lo, hi in BINNED_LONG_RUNS:     # identical rows that fill a row of 16 lanes / lie strictly inside one: the late steps of the segmented sums
        x[lo:hi] = x[lo]
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def binned_inputs(name):
    """[B, 3] float32, read-only.  A: the 4999 ray-ordered rows.  B: the same, plus for every level whose last bucket holds one row two points with a corner
    on that row (found by search: a plain draw of 4999 touches such a row 0-2 times).  C: 40000 points uniform in a cube of 8 cells of level 2 from 0.40."""
    if name == "C":
        scale, _ = oracle.grid_level_params(BINNED_A[0], BINNED_A[2], BINNED_A[1])
        return _frozen((0.40 + np.random.default_rng(2).random((40000, 3)) * (8.0 / float(scale[2]))).astype(np.float32))
    if name[0] == "A":
        return _binned_rays()
    L_, H_, pls, offsets, gridtype, ac = binned_case(name)
    rng = np.random.default_rng(70001 + gridtype)
    want = {l: int(offsets[l + 1]) - 1 for l in range(L_) if int(offsets[l + 1] - offsets[l]) % BIN_ROWS == 1}
    found = {l: [] for l in want}
    for _ in range(40):
        cand = rng.random((50000, 3)).astype(np.float32)
        ref = GridReference(cand, offsets, pls, H_, gridtype, ac)
        for l, row in want.items():
            found[l] += list(cand[(ref.rows[l] == row).any(axis=0)][: 2 - len(found[l])])
        if all(len(v) == 2 for v in found.values()):
            break
    assert all(len(v) == 2 for v in found.values()), "no point found on a one-row last bucket"
    return _frozen(np.concatenate([_binned_rays()] + [np.stack(found[l]) for l in sorted(found)]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def binned_grad(name):
    """[B, L * 2] float32, read-only: the output gradient a training step hands the table gradient.  Standard normal, then on the ray-ordered rows every
    seventh sample loses channel 0 only (it still contributes), ~5 % of the (sample, level) pairs are exactly zero, every segment is exactly zero on all
    levels from a random sample on (what the composite's backward writes behind a ray's stopping sample), and a few entries are -0.0 -- alone (the sample
    lives on) and as a pair (it is dead); the samples of BINNED_LONG_RUNS live on every level.  Rows appended to the rays (geometry B) and geometry C stay alive on every level."""
    L_ = binned_case(name)[0]
    B = binned_inputs(name).shape[0]
    rng = np.random.default_rng(1234 + BINNED_CASES.index(name))
    g = rng.standard_normal((B, L_, 2)).astype(np.float32)
    g[::7, :, 0] = 0.0
    if name != "C":
        g[:BINNED_RAYS][rng.random((BINNED_RAYS, L_)) < 0.05] = 0.0
        stop = rng.integers(1, 28, 185)                        # 27: the whole segment lives
        seg = g[:4995].reshape(185, 27, L_, 2)
        seg[np.arange(27)[None, :] >= stop[:, None]] = 0.0
        for i in range(40, BINNED_RAYS, 97):
            g[i, i % L_, 0] = -0.0                             # with channel 1 as it is
        for i in range(55, BINNED_RAYS, 131):
            g[i, i % L_] = -0.0                                # both channels: a dead sample
        for lo, hi in BINNED_LONG_RUNS:
            g[lo:hi] = rng.standard_normal((hi - lo, L_, 2)).astype(np.float32)
    return _frozen(g.reshape(B, L_ * 2))


@functools.lru_cache(maxsize=3)
def binned_reference(name, rows=None):
    """(GridReference, float64 table gradient, sum |w g|, addends per row) of a case, of its first `rows` samples if given; shared, not to be written"""
    L_, H_, pls, offsets, gridtype, ac = binned_case(name)
    x, g = binned_inputs(name), binned_grad(name)
    if rows is not None:
        x, g = x[:rows], g[:rows]
    ref = GridReference(x, offsets, pls, H_, gridtype, ac)
    return (ref,) + tuple(_frozen(a) for a in ref.table_grad(g))


def table_grad_accumulate_bound(D, mag, n, want, before):
    """The entry point added the gradient to `before` = p (fp32): one more rounding, of the sum: u |p + gradient|.  That is the whole statement for the
    image reduce and for a gather job that owns its bucket (one add per element).  A bucket split into j jobs adds j times: the last add rounds
    u |p + gradient| as before, each of the j - 1 earlier ones at most u (|p| + S) -- where table_grad_bound's derivation counted u S for it on a
    buffer of zeros.  With |p| <= S those 2 (j - 1) u S fit into the n u S of the bound from n >= 2 j - 1 on, so a test keeps |p| <= S on the
    rows that receive addends (and j <= 3 there)."""
    return table_grad_bound(D, mag, n) + U32 * np.abs(np.asarray(before, np.float64) + want)


def binned_live(ref, grad):
    """[L, B] bool: the (level, sample) pairs that write records -- inside [0, 1]^3 and a gradient that is not exactly zero"""
    g = np.asarray(grad).reshape(ref.B, ref.L, -1)
    return ref.inr[None, :] & (g != 0).any(axis=2).T


def binned_bucket_records(ref, grad, offsets, level):
    """records per bucket of `level` before any merging: 8 per live sample, by the bucket of each corner's row"""
    live = binned_live(ref, grad)[level]
    local = ref.rows[level][:, live] - int(offsets[level])
    return np.bincount((local // BIN_ROWS).reshape(-1), minlength=-(-int(offsets[level + 1] - offsets[level]) // BIN_ROWS))


def deleted_sample_ratio(ref, grad, bound, level, sample):
    """error / bound of a table gradient that lacks `sample`'s contribution on `level`: max over its eight rows of |w g| / bound (rows that two of its
    corners share are summed)"""
    g = np.asarray(grad, np.float64).reshape(ref.B, ref.L, -1)[sample, level]
    w = ref._weights(level, np.arange(1 << ref.D))[:, sample]
    rows = ref.rows[level, :, sample]
    worst = 0.0
    for r in np.unique(rows):
        miss = np.abs(w[rows == r].sum() * g)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(miss == 0, 0.0, miss / bound[r])
        worst = max(worst, float(q.max()))
    return worst
