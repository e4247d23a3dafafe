"""MI355X-first fused evaluation of the fields (no reference counterpart as one call): level-major
hash-grid lookup feeding the MFMA tiny-MLP kernel directly, no permute/copy, no per-layer launches."""
import contextlib
import ctypes
import math
import os
import threading
import warnings

import numpy as np
import torch

from . import _lib
from ._torch_glue import call, ptr, require, stream_ptr

_u32, _f32, _int = ctypes.c_uint32, ctypes.c_float, ctypes.c_int


def grid_encode_raw(encoder, x01):
    """[B,3] in [0,1] -> raw level-major [L,B,C] fp32 encoder output (the layout the kernels produce)."""
    B = x01.shape[0]
    L, C = encoder.num_levels, encoder.level_dim
    out = torch.empty(L, B, C, device=x01.device, dtype=torch.float32)
    emb = encoder.embeddings.detach()
    call("pnr_grid_encode_forward", ptr(require(x01, torch.float32, "inputs")), ptr(require(emb, torch.float32, "embeddings")),
         ptr(encoder.offsets), ptr(out), _u32(B), _u32(encoder.input_dim), _u32(C), _u32(L), _f32(np.log2(encoder.per_level_scale)),
         _u32(encoder.base_resolution), None, _u32(encoder.gridtype_id), _int(int(encoder.align_corners)), _int(0), units=B)
    return out


def _no_pair_copy():
    return None


class _PairCopy:
    """The interleaved [rows][2][2] copy of two encoders' tables that the training pair lookup reads.  It lives ON the first encoder (attribute
    `_pnr_pair`: freed with the model, no global registry, no id() aliasing after a model is freed) and remembers its partner by weak reference.
    A half is re-copied when torch can tell its table changed (_pkey: Parameter identity, storage, version -- optimiser steps, load_state_dict,
    in-place ops).  Writes through `.data` move none of those: invalidate_fused_caches(model) drops the copy (load_state_dict and
    initialize_palette call it), and as a safety net every call leaves a sampled checksum of both tables (pnr_checksum, one tiny launch, read
    back asynchronously) that the NEXT call compares with the one taken when the copy was made -- a silent `.data` rewrite is therefore noticed
    one call late, the copy rebuilt and a warning raised; PNR_PARANOID_CACHE=1 rebuilds on every call."""

    def __init__(self, enc_b, ea):
        import weakref
        self.partner = weakref.ref(enc_b)
        self.keys = [None, None]
        self.table = torch.empty(ea.shape[0], 2, 2, dtype=torch.float32, device=ea.device)
        self.sum_dev = torch.zeros(2, dtype=torch.int64, device=ea.device)
        self.sum_host = torch.zeros(2, dtype=torch.int64).pin_memory()
        self.sum_event = None       # recorded behind the asynchronous read-back of the last call's checksums
        self.sum_ref = [None, None]  # checksums of the tables as they were when their halves were copied

    # a copy or a pickle of the encoder (copy.deepcopy(model), torch.save(model)) does not take the derived table along: the copy rebuilds its own
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_pair_copy, ())

    def matches(self, enc_b, ea):
        return self.partner() is enc_b and self.table.device == ea.device and self.table.shape[0] == ea.shape[0]

    def lagged_check(self):
        """Look at the previous call's checksums (complete by now: a whole training step lies between two calls); a half whose table was rewritten
        behind torch's counters is marked stale."""
        if self.sum_event is None:
            return
        self.sum_event.synchronize()
        now = self.sum_host.tolist()
        self.sum_event = None
        for i in (0, 1):
            if self.sum_ref[i] is None:
                self.sum_ref[i] = now[i]
            elif self.sum_ref[i] != now[i]:
                warnings.warn("pair lookup: a hash table was rewritten behind torch's version counters (a `.data` write) -- the interleaved copy "
                              "was stale for one call; call invalidate_fused_caches(model) after such writes")
                self.keys[i] = None
                self.sum_ref[i] = None

    def refresh(self, tabs):
        with torch.no_grad():       # only the half whose table has changed (PaletteNeRF training: the density table is frozen)
            for i, t in enumerate(tabs):
                k = _pkey(t)
                if self.keys[i] != k or PARANOID:
                    self.table[:, i].copy_(t.detach())
                    self.keys[i] = k
                    self.sum_ref[i] = None      # the checksum this call takes becomes the reference
        n = 2
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tabs])
        sizes = (ctypes.c_uint64 * n)(*[t.numel() * t.element_size() for t in tabs])
        strides = (_u32 * n)(*[TABLE_CHECK_STRIDE] * n)
        call("pnr_checksum", ptrs, sizes, strides, _u32(n), ptr(self.sum_dev))
        self.sum_host.copy_(self.sum_dev, non_blocking=True)
        self.sum_event = torch.cuda.Event()
        self.sum_event.record()


def drop_pair_copies(model):
    """Forget the training pair lookup's interleaved table copies held by the model's encoders (see _PairCopy)."""
    for name in ("encoder", "encoder_palette", "encoder_clip"):
        enc = getattr(model, name, None)
        if enc is not None and "_pnr_pair" in getattr(enc, "__dict__", {}):
            del enc.__dict__["_pnr_pair"]


def grid_encode_raw_pair(enc_a, enc_b, x01):
    """Two hash-grid encoders of the same geometry at the same points in one launch (pnr_grid_encode_forward_pair): returns their two raw
    level-major [L,B,2] outputs, each bit for bit what grid_encode_raw gives.  The tables are read from an interleaved copy [rows][2][2] that is
    rebuilt (one strided copy, ~30 us for 2 x 49 MB) whenever either parameter has changed since -- every optimiser step in training, where the pair
    still costs ~1.3 lookups + that copy instead of 2 lookups.  The copy's life and staleness rules: _PairCopy."""
    ea, eb = enc_a.embeddings, enc_b.embeddings
    hit = enc_a.__dict__.get("_pnr_pair")
    if hit is None or not hit.matches(enc_b, ea):
        hit = _PairCopy(enc_b, ea)
        enc_a.__dict__["_pnr_pair"] = hit      # (__dict__: a plain attribute, not a registered buffer -- it must stay out of state_dict)
    hit.lagged_check()
    hit.refresh((ea, eb))
    return _encode_pair(enc_a, hit.table, x01)


def _encode_pair(enc_a, pair, x01):     # pnr_grid_encode_forward_pair over an interleaved [rows][2][2] fp32 table of two encoders of enc_a's geometry -> two raw [L,B,2] outputs
    B, L = x01.shape[0], enc_a.num_levels
    out0 = torch.empty(L, B, 2, device=x01.device, dtype=torch.float32)
    out1 = torch.empty(L, B, 2, device=x01.device, dtype=torch.float32)
    call("pnr_grid_encode_forward_pair", ptr(require(x01, torch.float32, "inputs")), ptr(pair), ptr(enc_a.offsets), ptr(out0), ptr(out1), _u32(B), _u32(L),
         _f32(np.log2(enc_a.per_level_scale)), _u32(enc_a.base_resolution), _u32(enc_a.gridtype_id), _int(int(enc_a.align_corners)), units=B)
    return out0, out1


def pairable(enc_a, enc_b):
    """Same geometry (offsets, levels, scales), fp32 tables with two features per level on one device: what the pair lookup needs."""
    try:
        return (enc_a.num_levels == enc_b.num_levels and enc_a.level_dim == 2 and enc_b.level_dim == 2 and enc_a.input_dim == 3 and enc_b.input_dim == 3
                and enc_a.per_level_scale == enc_b.per_level_scale and enc_a.base_resolution == enc_b.base_resolution and enc_a.gridtype_id == enc_b.gridtype_id
                and enc_a.align_corners == enc_b.align_corners and enc_a.embeddings.shape == enc_b.embeddings.shape
                and enc_a.embeddings.dtype == torch.float32 and enc_b.embeddings.dtype == torch.float32 and enc_a.embeddings.device == enc_b.embeddings.device
                and enc_a.embeddings.is_cuda)
    except AttributeError:
        return False


def tile_ray_order(pixel_index, W, tile=8):
    """Permutation that visits rays tile by tile (tile x tile pixels, row-major inside a tile): one wave = one 8x8 tile.
    pixel_index: int64 [N] row-major pixel id of every ray (arange(H*W) for a full frame, the shard's ids otherwise)."""
    y, x = pixel_index // W, pixel_index % W
    if tile == 0:                                   # full Z-order over pixels
        def spread(v):
            v = (v | (v << 8)) & 0x00FF00FF
            v = (v | (v << 4)) & 0x0F0F0F0F
            v = (v | (v << 2)) & 0x33333333
            return (v | (v << 1)) & 0x55555555
        return torch.argsort(spread(x) | (spread(y) << 1)).to(torch.int32)
    key = ((y // tile) * ((W + tile - 1) // tile) + (x // tile)) * (tile * tile) + (y % tile) * tile + (x % tile)
    return torch.argsort(key).to(torch.int32)


PARANOID = os.environ.get("PNR_PARANOID_CACHE") == "1"   # rebuild every derived blob on every use (debugging aid for code that writes through `.data`)


_held_keys = threading.local()     # .memo: {id(tensor): key} while a frame / field call holds its answers (_PrecisionGuard._held), else absent / None


def _pkey(p):
    """Identity of a parameter's CURRENT value as far as torch can tell: the Parameter object, its storage and its version counter.
    In-place torch ops, optimizer steps and load_state_dict bump the version; replacing the Parameter changes the identity.  Writes through
    `p.data` (torch_ema's copy_to / restore, `p.data.uniform_()`) change neither: call invalidate_fused_caches(model) after those.
    Inside a held call a tensor's key is formed once (the source watch, the guard and the packer each ask for the same twenty tensors)."""
    memo = getattr(_held_keys, "memo", None)
    if memo is None:
        return (id(p), p.data_ptr(), p._version)
    k = memo.get(id(p))
    if k is None:
        k = memo[id(p)] = (id(p), p.data_ptr(), p._version)
    return k


def _weight_of(module, *path):
    """module.<path[0]>[path[1]]....weight through the modules' own dictionaries: what `m.sigma_net[0].weight` returns, without nn.Module.__getattr__'s
    fallback chain and ModuleList's index arithmetic per step (a frame asks for a dozen weights; the walk was a tenth of its host time)."""
    for name in path:
        module = module._modules[str(name)]
    return module._parameters["weight"]


def invalidate_fused_caches(model):
    """Forget every blob derived from the model's parameters (packed MFMA weights, interleaved / half tables, host-side parameter copies).
    Called by load_state_dict and initialize_palette; call it yourself after writing parameters through `.data` (EMA swap-in / restore:
    nerf/utils.py:829-839, 959-961).  Whole-tensor `.data` rewrites are also caught by the per-frame checksum (_SourceWatch); a write to only
    PART of a hash table is not (tables are checksummed on every 1 021st word): after such a write this call is required."""
    for attr in ("_fused", "_density_fused", "_bg_fused"):
        f = getattr(model, attr, None)
        if f is not None:
            f.invalidate_caches()
    drop_pair_copies(model)
    for ref in list(model.__dict__.get("_fused_twins", [])):      # handles made by pipeline.clone_for_concurrent_frames: same weights, own blobs
        twin = ref()
        if twin is not None and twin is not model:
            invalidate_fused_caches(twin)


class _Derived:
    """Everything a fused object derives from parameters and settings (packed weight blobs, half / interleaved tables, the guard's bounds, the edit struct, the
    frame call's kept argument struct, the checksum call's argument arrays): slot -> (key, value).  THE RULES, stated here once:
      * a value is valid while its key is unchanged: the _pkey of every source (identity, storage, version), the settings it was built for and, where the
        sources' keys do not already say so, the device;
      * a rebuild is a NEW object.  The cache never writes into a value it has handed out: a prepared or submitted frame holds the old one (its token keeps it);
      * PNR_PARANOID_CACHE=1 rebuilds on every use (get() is the only place that reads PARANOID for one of these slots);
      * invalidate_caches() of the owner clears every slot; a frame that finds sources moved drops the slots derived from THEM (_SourceWatch._watch_begin).
        Both bump `_gen`, by which a frame prepared earlier is recognised (StaleFrame);
      * a copy or a pickle of the owner carries no values along and rebuilds its own (as _PairCopy)."""
    def __init__(self):
        self._slots = {}

    def get(self, slot, key, build, *args):
        """The stored value of `slot` while its key is `key`, else build(*args), a NEW object (a function and its arguments, not a closure: most calls are hits)."""
        hit = self._slots.get(slot)
        if hit is None or hit[0] != key or PARANOID:
            hit = self._slots[slot] = (key, build(*args))
        return hit[1]

    def key(self, slot):
        return self._slots.get(slot, (None, None))[0]

    def peek(self, slot):
        return self._slots.get(slot, (None, None))[1]

    def slots(self):
        return list(self._slots)

    def clear(self):
        self._slots = {}

    def drop(self, pkeys):     # forget every slot whose key holds one of these source keys, at any depth
        holds = lambda k: k in pkeys or (type(k) is tuple and any(holds(x) for x in k))
        self._slots = {s: kv for s, kv in self._slots.items() if not holds(kv[0])}

    def __deepcopy__(self, memo):
        return _Derived()

    def __reduce__(self):
        return (_Derived, ())


class _FusedState:
    """The fused objects' state, declared in one place (the mixins below have no constructor): every constructor calls _init_state().  `_cache`: see _Derived."""

    def _init_state(self):
        self._cache = _Derived()
        self._gen = 0                 # invalidations and precision changes so far: frames prepared before the last one are refused (StaleFrame)
        self._slot = 1                # the argument struct / read-back row of the frame prepared last (two alternate)
        self._handed = None           # the slot of the blob handed out last (`packed` / `versions`)
        self._overflowed_key = None   # the guard key of the weights that left fp16's range under the watch
        self._watch_keys = self._watch_ref = None     # _SourceWatch: the sources' keys at the last frame; (keys, checksums) of the reference
        self._watch_dev = self._watch_host = self._watch_rows = None     # its read-back buffers and their two rows
        self._guard_hold = False      # _PrecisionGuard._held: inside a held call, and the answers held for it
        self._guard_held = self._weights_held = None
        self._ws = None               # the frame call's workspace
        self.ray_order = None         # setting: a permutation of the rays (tile_ray_order)
        self.time_grid_kernel = False  # bench.py: HIP-event timing of the grid-encode launches inside the native frame loop

    packed = property(lambda self: self._cache.peek(self._handed), doc="the weight blob handed out last (None after an invalidation)")
    versions = property(lambda self: self._cache.key(self._handed), doc="its key: (device, the _pkey of every source, precision)")

    def invalidate_caches(self):
        self._cache.clear()
        self._watch_ref = None       # the next frame rebuilds every blob: its source checksums become the reference
        self._guard_held = self._weights_held = None   # (a held call that retries asks again)
        self._gen += 1               # frames prepared before this point hold pointers into the old blobs (frame_launch refuses them)

    _to_half = staticmethod(lambda t: t.to(torch.float16).contiguous())

    def _half_table(self, t):     # the reference's `embeddings.to(torch.half)` per forward (gridencoder/grid.py:38), converted once per update here
        return self._cache.get("half_table", _pkey(t), self._to_half, t)


F16X3_SAFE_ACTIVATION = 3.0e4   # fp16 overflows at 65 504: above this bound on any split operand the field runs on the exact fp32 path
F16X3_MAX_WEIGHT = 6.0e4        # the weights are split into fp16 halves at pack time: one beyond this cannot be represented at all


def _l1(w):
    """max_j sum_i |W[j][i]|: the factor by which a dense layer can grow the largest |activation|."""
    return w.detach().abs().sum(dim=1).max()


def _prescale_of(table_max):
    """Power of two that lifts a table's largest |entry| into [0.5, 1) when it is below 1/8 (else 1): below that the `lo` halves of the
    split features start to fall into fp16's subnormal range (the reference initialises its tables U(-1e-4, 1e-4), gridencoder/grid.py:107)."""
    if not math.isfinite(table_max) or table_max <= 0.0 or table_max >= 0.125:
        return 1.0
    return float(2.0 ** min(14, math.floor(-math.log2(table_max))))


class _PrecisionGuard:
    """What the split-fp16 matrix path needs to be safe for ANY weights: operands are split into two fp16 halves, so
    (a) very small encoder features lose their low half to the subnormal range -> they are pre-multiplied by a power of two inside the kernel
        (enc_scale, exact: the first stack is bias-free and positively homogeneous; undone on its outputs);
    (b) an activation beyond fp16's range becomes inf -> a static bound on every split operand (largest table entry times the layers' L1 row
        norms) is computed when the blob is (re)packed; if it can exceed F16X3_SAFE_ACTIVATION the call runs on the exact fp32 path instead.
    `precision` is what the caller asked for; `effective_precision()` is what runs.  A handful of tiny device reductions and ONE host read per
    repack (never per frame)."""

    def _guard_tables(self):
        raise NotImplementedError

    def _guard_weights(self):
        return self._w()

    def _blob_sources(self):     # the tensors the packed blob is derived from: the weights that run, and what a field packs next to them
        return self._guard_weights()

    def _guard_bound(self, tmax, scales):
        raise NotImplementedError

    @contextlib.contextmanager
    def _held(self):
        """Context manager for one call of the stand-alone ops: the guard is evaluated once and its answer held until the call returns (effective_precision,
        enc_scales and _pack each ask; every answer walks the model's parameters -- 36 % of the host time of a drop-in frame with dropin.fuse_field)."""
        self._guard_hold = True
        outer = getattr(_held_keys, "memo", None)     # (a thread-local: absent in a thread's first call)
        if outer is None:
            _held_keys.memo = {}
        try:
            yield
        finally:
            self._guard_hold = False
            self._guard_held = self._weights_held = None
            if outer is None:
                _held_keys.memo = None

    def _w(self):
        """self._weights(), looked up once per held call (a dozen nn.Module attribute walks, asked for by the guard, the packer and the source watch)."""
        if self._weights_held is not None:
            return self._weights_held
        ws = self._weights()
        if self._guard_hold:
            self._weights_held = ws
        return ws

    def _guard(self):     # -> (enc scales, static bound, largest |weight|): the "guard" slot, keyed on the weights and tables it is computed from
        if self._guard_held is not None:
            return self._guard_held
        tables = self._guard_tables()
        key = tuple(_pkey(w) for w in self._guard_weights()) + tuple(_pkey(t) for t in tables)
        state = self._cache.get("guard", key, self._guard_build, tables)
        if self._guard_hold:
            self._guard_held = state
        return state

    def _guard_build(self, tables):
        tmax = [float(v) for v in torch.stack([t.detach().abs().max().float() for t in tables]).cpu().tolist()]
        scales = [_prescale_of(v) for v in tmax]
        bound = float(self._guard_bound(tmax, scales))
        wmax = float(torch.stack([w.detach().abs().max().float() for w in self._guard_weights()]).max())   # the weights are split into fp16 halves too
        return (scales + [1.0] * (3 - len(scales)), bound, wmax)

    def _pack(self, prec=None):
        """The MFMA-ordered weight blob for `prec`, slot ("blob", prec): one blob per precision (the stand-alone ops may run fp32 where the frame loops run
        split-fp16 with the watch, and a frame prepared or in flight at one precision must never see the other's layout); _pack_build(prec) packs a new one."""
        prec = self.effective_precision() if prec is None else prec
        srcs = self._blob_sources()
        self._handed = slot = ("blob", prec)
        return self._cache.get(slot, (srcs[0].device,) + tuple(_pkey(t) for t in srcs) + (prec,), self._pack_build, prec)

    def enc_scales(self, prec=None):
        """[s_encoder, s_encoder_palette, s_encoder_clip] for the split-fp16 path (all 1.0 on the fp32 path)."""
        prec = self.effective_precision() if prec is None else prec
        return self._guard()[0] if prec in (1, 2) else [1.0, 1.0, 1.0]

    def _fp16_level(self):
        """1 = PNR_FIELD_F16X3 (split operands), 2 = PNR_FIELD_F16X2 (opt-in, NeRF field only: activations rounded once to fp16)."""
        return 2 if int(self.precision) == 2 and getattr(self, "supports_f16x2", False) else 1

    def effective_precision(self):
        """Matrix path of the stand-alone ops: an fp16 form only when the static bound rules an fp16 overflow out."""
        if int(self.precision) == 0:
            return 0
        return self._fp16_level() if self._guard()[1] < F16X3_SAFE_ACTIVATION and self._guard()[2] < F16X3_MAX_WEIGHT else 0

    def frame_precision(self):
        """(precision, watch) for the device-driven frame loops.  The static bound is a guarantee but pessimistic (products of L1 norms): trained
        weights often fail it without ever coming near fp16's range.  The frame loops therefore keep split-fp16 in that case and let the
        kernels WATCH the operands they split (watch = True, ~1 VALU per operand); a frame that reports an overflow is rendered again in exact
        fp32, and these weights stay on fp32 from then on (render_frame)."""
        if int(self.precision) == 0 or not self._guard()[2] < F16X3_MAX_WEIGHT:   # a weight itself beyond fp16's range: nothing to watch for
            return 0, False
        if self._guard()[1] < F16X3_SAFE_ACTIVATION:
            return self._fp16_level(), False
        if self._overflowed_key is not None and self._overflowed_key == self._cache.key("guard"):
            return 0, False
        return self._fp16_level(), True

    def _note_overflow(self):
        self._overflowed_key = self._cache.key("guard")
        self._gen += 1     # frames prepared before this point carry split-fp16 and the watch in their structs: frame_launch refuses them (StaleFrame), render_launch prepares them again
        warnings.warn("fused field: an activation left fp16's range (> 65504) in the split-fp16 matrix path: the frame is rendered again on the exact "
                      "fp32 path, which these weights keep from now on")


TABLE_CHECK_STRIDE = 1 if PARANOID else 1021   # hash tables are checksummed on every 1021st word per frame (12 k scattered words of a 50 MB table: ~3 us; every 61st cost 18 us); weights in full


def _checksum_args(srcs):     # pnr_checksum's three argument arrays for [(tensor, stride in 4-byte words)]
    return ((ctypes.c_void_p * len(srcs))(*[t.data_ptr() for t, _ in srcs]), (ctypes.c_uint64 * len(srcs))(*[t.numel() * t.element_size() for t, _ in srcs]),
            (_u32 * len(srcs))(*[int(st) for _, st in srcs]))


class _SourceWatch:
    """Blobs derived from parameters go stale SILENTLY when the parameters are rewritten through `.data` (torch_ema's copy_to / restore around
    an evaluation, nerf/utils.py:829-839, 959-961): neither identity nor version moves, so the keys above cannot tell.  The frame loops
    therefore checksum the sources on the device once per frame (pnr_checksum: one small launch, 8 bytes per source back with the frame's own
    read-back) and compare with the checksums taken when the blobs were built; on a mismatch the blobs are rebuilt and the frame is rendered
    again.  When torch CAN tell (a key changed), what derives from the sources that moved is rebuilt in that frame -- also what was built since the
    move -- and only THEIR checksums become the new reference: the other sources are still compared, so a `.data` write cannot hide behind another
    source's version bump (it gives the warning and the second render).  Tables are sampled (TABLE_CHECK_STRIDE): a swap or a re-initialisation
    touches every row and is caught.  LIMITATION: a `.data` write that touches only PART of a table (loading or pruning some levels, a partial
    re-initialisation) will usually miss the sampled words and is NOT detected -- call invalidate_fused_caches(model) after such a write, or
    run with PNR_PARANOID_CACHE=1, which checks every word."""

    def _watched(self):
        """[(tensor, stride in 4-byte words)]: everything a cached blob of this object is derived from."""
        raise NotImplementedError

    def _watch_begin(self, slot=0):
        """slot: 0 / 1 -- a frame prepared while the previous one is still running (frame_prepare / frame_launch / frame_finish) takes the other read-back row."""
        srcs = self._watched()
        keys = tuple(_pkey(t) for t, _ in srcs)
        had = self._watch_keys
        if had == keys:
            keys = had         # (the same OBJECT while nothing moves: _watch_end and the plan key then compare by identity)
        elif had is not None:      # (an object's sources are the same tensors' places for life: the two tuples pair up)
            self._cache.drop({k for pair in zip(had, keys) if pair[0] != pair[1] for k in pair})
            self._gen += 1           # frames prepared before this point hold pointers into the old blobs (frame_launch refuses them)
        self._watch_keys = keys
        n, dev = len(srcs), srcs[0][0].device
        if self._watch_dev is None or self._watch_dev.device != dev or self._watch_dev.shape[1] < n:
            self._watch_dev = torch.zeros(2, max(n, 24), dtype=torch.int64, device=dev)
            self._watch_host = torch.zeros(2, max(n, 24), dtype=torch.int64).pin_memory()
            self._watch_rows = [(self._watch_dev[k], self._watch_host[k]) for k in (0, 1)]     # (row views made once: a view per frame is host time)
        ptrs, sizes, strides = self._cache.get("watch_args", keys, _checksum_args, srcs)     # (the keys hold the data pointers: same keys, same argument arrays)
        drow, hrow = self._watch_rows[slot]
        call("pnr_checksum", ptrs, sizes, strides, _u32(n), ptr(drow))
        hrow.copy_(drow, non_blocking=True)     # complete once the frame's own read-back is (same stream)
        return self._watch_ref is None, keys, slot

    def _watch_end(self, state):
        """True: the frame just rendered used blobs that match their sources."""
        record, keys, slot = state
        sums = tuple(self._watch_rows[slot][1][:len(keys)].tolist())
        ref = self._watch_ref            # (keys, checksums) as recorded
        if not record:
            if ref is None or keys is not self._watch_keys:      # invalidated, or a source moved, under the frame
                return False
            if keys is ref[0]:
                return sums == ref[1]
            have = dict(zip(*ref))      # a source whose key the reference holds must have its checksum; one that moved since gets its reference here
            if any(have.get(k, c) != c for k, c in zip(keys, sums)):
                return False
        self._watch_ref = (keys, sums)
        return True

    def _watch_failed(self):
        warnings.warn("fused field: parameters were rewritten behind torch's version counters (a `.data` write); the packed blobs were rebuilt and "
                      "the frame rendered again -- invalidate_fused_caches(model) after such writes avoids the double render")
        self.invalidate_caches()


def _set_near_far(a, nears, fars, aabb, min_near, N, dev):
    """nears / fars of a frame-args struct: given, or (aabb set, both None) left to the frame call's first launch (pnr_nerf_frame_args::aabb)."""
    a.aabb = None
    if nears is None or fars is None:
        if aabb is None:
            raise RuntimeError("render_frame needs nears / fars or the box they follow from (aabb)")
        if not (aabb.is_cuda and aabb.dtype == torch.float32 and aabb.is_contiguous() and aabb.numel() == 6):
            raise RuntimeError("aabb must be 6 contiguous fp32 values on the device")
        nears = torch.empty(N, dtype=torch.float32, device=dev)
        fars = torch.empty(N, dtype=torch.float32, device=dev)
        a.aabb, a.min_near = aabb.data_ptr(), float(min_near)
    a.nears, a.fars = nears.data_ptr(), fars.data_ptr()
    return nears, fars


def _set_finish(a, bg_color, N, mask):
    """Fill the finish / bg fields of a frame-args struct; returns True when the call will apply the epilogue."""
    a.finish, a.bg_map = 0, None
    if bg_color is None:
        return False
    if torch.is_tensor(bg_color):
        if bg_color.numel() == 3:
            vals = [float(v) for v in bg_color.flatten().tolist()]
        elif bg_color.shape[-1] == 3 and bg_color.numel() == 3 * N and bg_color.is_cuda and bg_color.dtype == torch.float32 and bg_color.is_contiguous():
            a.bg_map = bg_color.data_ptr()
            vals = [0.0, 0.0, 0.0]
        else:
            return False
    elif isinstance(bg_color, (int, float)):
        vals = [float(bg_color)] * 3
    else:
        vals = [float(v) for v in bg_color]
        if len(vals) != 3:
            return False
    for k in range(3):
        a.bg_color[k] = vals[k]
    a.finish = mask
    return True


def _noises_ptr(noises, N, dev):
    """The `noises` field of a frame-args struct: None, or the address of N contiguous fp32 values on the frame's device (the token keeps the tensor)."""
    if noises is None:
        return None
    if not (torch.is_tensor(noises) and noises.dtype == torch.float32 and noises.device == dev and noises.is_contiguous() and noises.numel() == N):
        raise RuntimeError("noises must be N contiguous fp32 values on the rays' device (one uniform draw per ray, indexed by ray id)")
    return noises.data_ptr()


class StaleFrame(RuntimeError):
    """frame_launch of a frame that was prepared before the object's blobs were rebuilt (invalidate_caches): prepare it again."""


class _FrameToken:
    """A frame between frame_prepare and frame_finish: the argument struct the C calls are given (`args`) and its pnr_nerf_frame_args part (`base`: the struct
    itself for a NeRF frame, its first member for a palette frame), outputs, host-side stats arrays and what a re-render needs."""
    __slots__ = ("args", "base", "out", "stats", "kms", "watch_state", "watch", "finished", "nears", "fars", "again", "keep", "stream", "depth_raw", "edit", "valid", "gen", "noises")

    def __init__(self, **kw):
        self.valid = None
        for k, v in kw.items():
            setattr(self, k, v)


def _frame_valid(fused, tok):
    """0: the finished frame's outputs stand; 1: its blobs did not match their sources (a `.data` write); 2: an operand left fp16's range under the watch."""
    if not fused._watch_end(tok.watch_state):
        return 1
    return 2 if (tok.watch and tok.stats[5]) else 0


class _FrameLoop:
    """The host side of the device-driven frame loop, once for both fields (as `render_frame_impl` in csrc/frame.hip is one function for both ABIs): the whole
    frame call, the same call in three steps, the kept argument struct, the two retries.  What a field class supplies:
      _frame_entry, _frame_finish_mask           its C entry points (looked up on the library object by name at every call: profiles/frame_host_time.py
                                                 wraps them there) and pnr_nerf_frame_args::finish for a call that applies the epilogue
      _frame_struct()                            -> (the struct the C calls are given, its pnr_nerf_frame_args part)
      _frame_key(m, enc)                         the plan key's terms for what _frame_fill reads
      _frame_workspace_bytes(lib, N)
      _frame_fill(args, a, m, enc)               the kept struct's table pointers and the fields only this kind has -> the tensors whose addresses it stored
      _frame_extras(tok, N, dev)                 per-frame outputs and struct fields only this kind has (the token is complete otherwise)
      _frame_outputs(tok, stats)                 the result tuple"""

    _frame_finish_mask = 3       # (7: the epilogue also goes over the palette frame's aux_map)

    def _frame_extras(self, tok, N, dev):
        pass

    def _frame_outputs(self, tok, stats):
        return tok.out + (stats,)

    @torch.no_grad()
    def render_frame(self, rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color=None, aabb=None, min_near=0.0, noises=None):
        """One inference frame through the device-driven loop (pnr_nerf_render_frame / pnr_palette_render_frame).  Returns
        (weights_sum [N], depth [N], image [N,3], stats dict); a palette field (weights_sum, depth, image, aux_map [N, aux_channels], stats).
        bg_color None: raw accumulations (bg mix and depth normalisation are the caller's); a number, 3 numbers or an [N,3] tensor: the call's last launch also
        applies run_cuda's epilogue (image + (1 - ws) bg, normalised depth; palette/renderer.py:520-540: also aux_map[:, 0:3] = direct_rgb blended with the
        background, the raw depth kept in stats['depth_raw']) -- stats['finished'] says so.  aabb (device tensor of 6 floats) with nears = fars = None: the call
        computes near / far in its first launch (near_far_from_aabb's arithmetic); stats['nears'], stats['fars'] hold them.  noises ([N] fp32 on the device, by ray
        id): the first-sample jitter of march_rays(perturb=True), applied in the frame's first iteration (pnr_nerf_frame_args::noises); None: no jitter."""
        with self._held():
            return self._render_frame(rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises)

    # The same frame in three steps (round 6; <entry>_submit / _finish): frame_prepare does everything in front of the library call (outputs, argument
    # struct, source checksums) and may run while the PREVIOUS frame is still on the device; frame_launch enqueues the frame and returns at once; frame_finish waits
    # for it and returns what render_frame returns.  A caller with a queue of frames (a video path, a rank's shard loop) runs
    #     tok = prepare(0); launch(tok);  for i in 1..: nxt = prepare(i); out = finish(tok); launch(nxt); tok = nxt; consume(out)
    # so that the host's work for frame i + 1 lies under frame i's kernels.  Two argument structs alternate (a frame's struct must stay as it was until its finish).
    @torch.no_grad()
    def frame_prepare(self, rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color=None, aabb=None, min_near=0.0, noises=None):
        with self._held():
            return self._frame_prepare(rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises)

    def frame_launch(self, tok):
        if tok.gen != self._gen:
            raise StaleFrame("the frame was prepared before the packed blobs were rebuilt")
        tok.stream = stream_ptr()
        name = self._frame_entry + "_submit"
        _lib.check(getattr(_lib.load(), name)(ctypes.byref(tok.args), tok.stream), name)
        return tok

    def frame_wait(self, tok):
        """The library's finish call alone: waits for the frame (and enqueues what it still needs).  True: the frame's outputs are valid -- the caller may enqueue
        its next frame before it asks for frame_result(); False: the frame has to be rendered again (sources rewritten behind torch's counters, an fp16
        overflow), which frame_result() does -- ask for it BEFORE launching another frame."""
        name = self._frame_entry + "_finish"
        _lib.check(getattr(_lib.load(), name)(ctypes.byref(tok.args), tok.stream), name)
        tok.valid = _frame_valid(self, tok)
        return tok.valid == 0

    @torch.no_grad()
    def frame_result(self, tok):
        with self._held():
            return self._frame_post(tok)

    def frame_finish(self, tok):
        self.frame_wait(tok)
        return self.frame_result(tok)

    def _render_frame(self, rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises=None):
        tok = self._frame_prepare(rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises)
        rc = getattr(_lib.load(), self._frame_entry)(ctypes.byref(tok.args), stream_ptr())
        _lib.check(rc, self._frame_entry)
        return self._frame_post(tok)

    def _frame_plan(self, N, dev, order, m, enc):
        """Everything of the argument struct that only changes when a parameter, a table or a setting does, filled once and kept (slot ("plan", 0 / 1): re-deriving
        these fifty values per frame was a third of the call's host time in front of the first launch) -> (args, its pnr_nerf_frame_args part, precision, watch, tensors it points at)."""
        nbytes = int(self._frame_workspace_bytes(_lib.load(), N))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        prec, watch = self.frame_precision()
        args, a = self._frame_struct()
        a.table_dtype = 1 if self.table_half else 0
        a.N = N
        a.bound, a.C, a.H = float(m.bound), int(m.cascade), int(m.grid_size)
        a.offsets = enc.offsets.data_ptr()
        a.num_levels, a.S, a.base_resolution, a.gridtype = enc.num_levels, float(np.log2(enc.per_level_scale)), enc.base_resolution, enc.gridtype_id
        a.field_precision, a.watch_overflow = int(prec), int(watch)
        for k, v in enumerate(self.enc_scales(prec)):
            a.enc_scale[k] = v
        a.density_scale = float(m.density_scale)
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), nbytes
        a.ray_order = order.data_ptr() if order is not None else None
        return args, a, prec, watch, (self._ws, order) + self._frame_fill(args, a, m, enc)

    def _frame_prepare(self, rays_o, rays_d, nears, fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises=None):
        from . import raymarching
        m = self.model
        N = rays_o.shape[0]
        dev = rays_o.device
        slot = self._slot = 1 - self._slot
        watch_state = self._watch_begin(slot)
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty(N, 3, dtype=torch.float32, device=dev)
        order = self.ray_order
        if order is not None and order.numel() != N:
            order = None
        enc = m.encoder
        plan_key = (self._watch_keys, N, dev, int(self.precision), bool(self.table_half), self._overflowed_key, None if order is None else (id(order), order.data_ptr()),
                    float(m.bound), int(m.cascade), int(m.grid_size), float(m.density_scale), enc.num_levels, enc.per_level_scale, enc.base_resolution, enc.gridtype_id,
                    self._frame_key(m, enc))
        args, a, prec, watch, kept = self._cache.get(("plan", slot), plan_key, self._frame_plan, N, dev, order, m, enc)
        # The packed blob is NOT part of the plan: it is looked up per frame (a key compare when nothing changed, see _pack) and the token keeps it alive
        blob = self._pack(prec)
        a.packed_weights = blob.data_ptr()
        mip = raymarching.occupancy_mip(m.density_bitfield, m.cascade, m.grid_size, m.bound)
        stats = (ctypes.c_uint64 * 6)()
        kms = (ctypes.c_float * 2)()
        a.rays_o, a.rays_d = rays_o.data_ptr(), rays_d.data_ptr()
        nears, fars = _set_near_far(a, nears, fars, aabb, min_near, N, dev)
        a.bitfield = m.density_bitfield.data_ptr()
        a.mip = mip.data_ptr() if mip is not None else None
        a.dt_gamma, a.max_steps, a.T_thresh = float(dt_gamma), int(max_steps), float(T_thresh)
        a.weights_sum, a.depth, a.image = ws.data_ptr(), depth.data_ptr(), image.data_ptr()
        a.stats = ctypes.cast(stats, ctypes.c_void_p)
        a.kernel_ms = ctypes.cast(kms, ctypes.c_void_p) if self.time_grid_kernel else None     # (bench.py sets it)
        finished = _set_finish(a, bg_color, N, self._frame_finish_mask)
        a.noises = _noises_ptr(noises, N, dev)
        for t, name in ((rays_o, "rays_o"), (rays_d, "rays_d"), (nears, "nears"), (fars, "fars")):
            require(t, torch.float32, name)
        tok = _FrameToken(gen=self._gen, args=args, base=a, out=(ws, depth, image), stats=stats, kms=kms, watch_state=watch_state, watch=watch, finished=finished,
                          nears=nears, fars=fars,
                          again=(rays_o, rays_d, None if aabb is not None else nears, None if aabb is not None else fars, dt_gamma, max_steps, T_thresh, bg_color, aabb, min_near, noises),
                          keep=(mip, bg_color, blob, kept), noises=noises)
        self._frame_extras(tok, N, dev)
        return tok

    def _frame_post(self, tok):
        valid = tok.valid if tok.valid is not None else _frame_valid(self, tok)
        if valid:
            (self._watch_failed if valid == 1 else self._note_overflow)()
            return self._render_frame(*tok.again)
        stats, kms = tok.stats, tok.kms
        return self._frame_outputs(tok, {"iterations": int(stats[0]), "rendered": int(stats[1]), "rows": int(stats[2]), "enqueued": int(stats[3]), "looks": int(stats[4]),
                                         "grid_ms": float(kms[0]), "grid_launches": int(kms[1]), "finished": tok.finished, "nears": tok.nears, "fars": tok.fars})


class BackgroundFused(_FusedState):
    """The background model of a bg_radius > 0 network as ONE launch per frame (pnr_background_forward: sphere coordinates, the 2-D lookup of
    `encoder_bg`, SH, bg_net, sigmoid), for inference batches.  The weight blob and, for the reference's -O mode, the half copy of the table are slots of
    the object's cache ("blob", "half_table": see _Derived); `state()` changes whenever one was or has to be rebuilt (renderer.render_launch looks at it).
    Training batches (train_from_rays / train_from_coords) use none of these caches: the launches read the parameters themselves."""

    def __init__(self, model):
        if not self.supported(model):
            raise RuntimeError("the fused background launch is specialised for the reference's background model (hashgrid 4 x 2 over 2-D, SH degree 4, bg_net 24 -> 64 -> 3)")
        self.model = model
        self._init_state()

    @staticmethod
    def supported(m):
        from .gridencoder import GridEncoder
        e, net = getattr(m, "encoder_bg", None), getattr(m, "bg_net", None)
        try:
            return (isinstance(e, GridEncoder) and e.input_dim == 2 and e.num_levels == 4 and e.level_dim == 2 and getattr(m.encoder_dir, "degree", 0) == 4
                    and net is not None and len(net) == 2 and m.num_layers_bg == 2 and m.hidden_dim_bg == 64
                    and tuple(net[0].weight.shape) == (64, 24) and tuple(net[1].weight.shape) == (3, 64) and net[0].bias is None and net[1].bias is None
                    and net[0].weight.dtype == torch.float32 and net[1].weight.dtype == torch.float32 and e.embeddings.dtype == torch.float32)
        except AttributeError:
            return False

    def _weights(self):
        return [_weight_of(self.model, "bg_net", 0), _weight_of(self.model, "bg_net", 1)]

    def state(self):
        """Identity of everything a launch reads, as far as torch can tell, and the number of invalidations so far."""
        return (self._gen,) + tuple(_pkey(w) for w in self._weights()) + (_pkey(self.model.encoder_bg.embeddings),)

    def _pack(self):
        ws = self._weights()
        return self._cache.get("blob", (ws[0].device,) + tuple(_pkey(w) for w in ws), self._pack_build, ws)

    def _pack_build(self, ws):
        blob = torch.empty(int(_lib.load().pnr_background_packed_bytes()) // 4, dtype=torch.float32, device=ws[0].device)
        call("pnr_background_pack", *[ptr(require(w.detach().contiguous(), torch.float32, "bg_net weight")) for w in ws], ptr(blob))
        return blob

    def _table(self, half):
        emb = self.model.encoder_bg.embeddings
        return (self._half_table(emb), 1) if half else (require(emb.detach(), torch.float32, "encoder_bg.embeddings"), 0)

    def _set_geometry(self, a, table, dtype):     # the fields of a Background(Train)Args that say where the table is and how the lookup, the SH and bg_net are shaped
        m, enc = self.model, self.model.encoder_bg
        a.embeddings, a.table_dtype, a.offsets, a.table_rows = table.data_ptr(), dtype, require(enc.offsets, torch.int32, "offsets").data_ptr(), int(table.shape[0])
        a.num_levels, a.level_dim, a.S, a.H = enc.num_levels, enc.level_dim, float(np.log2(enc.per_level_scale)), enc.base_resolution
        a.gridtype, a.align_corners = enc.gridtype_id, int(enc.align_corners)
        a.sh_degree, a.num_layers, a.hidden_dim = int(m.encoder_dir.degree), int(m.num_layers_bg), int(m.hidden_dim_bg)

    @torch.no_grad()
    def _launch(self, rays_o, rays_d, coords, want_coords, half):
        m = self.model
        rays_d = require(rays_d.reshape(-1, 3).contiguous(), torch.float32, "rays_d")
        N, dev = rays_d.shape[0], rays_d.device
        half = torch.is_autocast_enabled() if half is None else bool(half)
        table, dtype = self._table(half)
        blob = self._pack()
        out = torch.empty(N, 3, dtype=torch.float32, device=dev)
        coords_out = torch.empty(N, 2, dtype=torch.float32, device=dev) if want_coords else None
        a = _lib.BackgroundArgs()
        a.N = N
        a.rays_d = rays_d.data_ptr()
        if coords is not None:
            coords = require(coords.reshape(-1, 2).contiguous(), torch.float32, "coords")
            if coords.shape[0] != N:
                raise RuntimeError("background: one coordinate pair per direction")
            a.coords_in = coords.data_ptr()
        else:
            rays_o = require(rays_o.reshape(-1, 3).contiguous(), torch.float32, "rays_o")
            if rays_o.shape[0] != N:
                raise RuntimeError("background: one origin per direction")
            a.rays_o, a.radius = rays_o.data_ptr(), float(m.bg_radius)
        self._set_geometry(a, table, dtype)
        a.packed, a.out = blob.data_ptr(), out.data_ptr()
        a.coords_out = coords_out.data_ptr() if coords_out is not None else None
        # (the launch is enqueued on torch's current stream before this returns: the caching allocator keeps `table`, `blob` and the inputs alive for it)
        call("pnr_background_forward", ctypes.byref(a), units=N)
        return (out, coords_out) if want_coords else out

    def from_rays(self, rays_o, rays_d, want_coords=False, half=None):
        """rays [N,3] -> background colour [N,3] (with want_coords: and the sphere coordinates [N,2], bit for bit raymarching.sph_from_ray's).
        half None: the half table under autocast, the fp32 table otherwise."""
        return self._launch(rays_o, rays_d, None, want_coords, half)

    def from_coords(self, x, d, half=None):
        """NeRFNetwork.background(x, d): x [N,2] the coordinates of sph_from_ray, d [N,3]."""
        return self._launch(None, d, x, False, half).view(*d.shape[:-1], 3)

    def _train_args(self, N, rays_d, coords, table):
        a = _lib.BackgroundTrainArgs()
        a.N, a.rays_d, a.coords_in = N, rays_d.data_ptr(), ptr(coords)
        self._set_geometry(a, table, 0)
        return a

    def _train(self, rays_o, rays_d, coords):
        """The training form: pnr_background_train_forward / pnr_background_backward behind one autograd.Function.  The table and the two weights are
        the model's parameters as they are at this call (no packed blob, no cache: an optimiser step or a write through `.data` is simply read)."""
        ws = self._weights()
        return _BackgroundTrain.apply(self, rays_o, rays_d, coords, self.model.encoder_bg.embeddings, ws[0], ws[1])

    def train_from_rays(self, rays_o, rays_d, want_coords=False):
        """from_rays with a gradient for encoder_bg.embeddings and bg_net's weights (none for the rays): rays [N,3] -> [N,3], fp32 also under autocast.
        want_coords: and the sphere coordinates [N,2] the backward will read."""
        out, coords = self._train(rays_o, rays_d, None)
        return (out, coords) if want_coords else out

    def train_from_coords(self, x, d):
        """from_coords with a gradient for the parameters (none for x or d)."""
        return self._train(None, d, x)[0].view(*d.shape[:-1], 3)


class _BackgroundTrain(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)   # under autocast: fp32 in, the fp32 table, fp32 out
    def forward(ctx, owner, rays_o, rays_d, coords, embeddings, w0, w1):
        f32 = torch.float32
        rays_d = require(rays_d.detach().reshape(-1, 3).contiguous(), f32, "rays_d")
        N, dev = rays_d.shape[0], rays_d.device
        table = require(embeddings.detach(), f32, "encoder_bg.embeddings")
        w0_, w1_ = (require(w.detach().contiguous(), f32, "bg_net weight") for w in (w0, w1))
        if coords is not None:
            coords = require(coords.detach().reshape(-1, 2).contiguous(), f32, "coords")
            if coords.shape[0] != N:
                raise RuntimeError("background: one coordinate pair per direction")
        out = torch.empty(N, 3, dtype=f32, device=dev)
        coords_out = torch.empty(N, 2, dtype=f32, device=dev)
        a = owner._train_args(N, rays_d, coords, table)
        if coords is None:
            rays_o = require(rays_o.detach().reshape(-1, 3).contiguous(), f32, "rays_o")
            if rays_o.shape[0] != N:
                raise RuntimeError("background: one origin per direction")
            a.rays_o, a.radius = rays_o.data_ptr(), float(owner.model.bg_radius)
        a.w0, a.w1, a.out, a.coords_out = w0_.data_ptr(), w1_.data_ptr(), out.data_ptr(), coords_out.data_ptr()
        call("pnr_background_train_forward", ctypes.byref(a), units=N)
        ctx.owner = owner
        ctx.save_for_backward(coords_out, rays_d, embeddings, w0, w1)
        ctx.mark_non_differentiable(coords_out)
        return out, coords_out

    @staticmethod
    @torch.autograd.function.once_differentiable      # no double backward: asking for one raises
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_rgb, _grad_coords):
        coords, rays_d, embeddings, w0, w1 = ctx.saved_tensors
        f32 = torch.float32
        N, dev = rays_d.shape[0], rays_d.device
        table = require(embeddings.detach(), f32, "encoder_bg.embeddings")
        w0_, w1_ = (require(w.detach().contiguous(), f32, "bg_net weight") for w in (w0, w1))
        g_w0, g_w1 = torch.empty_like(w0_), torch.empty_like(w1_)
        g_table = torch.zeros_like(table) if ctx.needs_input_grad[4] else None
        if N == 0:
            return None, None, None, None, g_table, g_w0.zero_(), g_w1.zero_()
        grad_rgb = require(grad_rgb.detach().reshape(-1, 3).float().contiguous(), f32, "grad_rgb")
        nbytes = int(_lib.load().pnr_background_backward_workspace_bytes(N))
        work = torch.empty(nbytes // 4, dtype=f32, device=dev)
        a = ctx.owner._train_args(N, rays_d, coords, table)
        a.w0, a.w1, a.grad_rgb, a.grad_w0, a.grad_w1, a.grad_table = w0_.data_ptr(), w1_.data_ptr(), grad_rgb.data_ptr(), g_w0.data_ptr(), g_w1.data_ptr(), ptr(g_table)
        a.workspace, a.workspace_bytes = work.data_ptr(), nbytes
        call("pnr_background_backward", ctypes.byref(a), units=N)
        return None, None, None, None, g_table, g_w0, g_w1


def background_train_fused(model, *inputs, fused_kernels=None):
    """The model's BackgroundFused for a TRAINING batch (train_from_rays / train_from_coords), or None: the per-op formulation stays.  The batch
    takes the fused path when gradients are enabled, the switch `model.fused_train_background` is on (the default), every input is an fp32 device
    tensor that needs no gradient itself, the model asked for fused kernels (the condition of the inference launch) and its background is the
    architecture the kernels support, with its parameters on the device.  fused_kernels: the caller's own answer to "asked for fused kernels"
    (dropin.fuse_field's binding is one)."""
    if not torch.is_grad_enabled() or not getattr(model, "fused_train_background", True):
        return None
    if fused_kernels is None:
        fused_kernels = bool(getattr(model, "fused_field", False)) or getattr(model, "march_mode", None) == "native"
    if not fused_kernels:
        return None
    for t in inputs:
        if not t.is_cuda or t.dtype != torch.float32 or t.requires_grad:
            return None
    f = background_fused(model)
    return f if f is not None and model.encoder_bg.embeddings.is_cuda else None


def background_fused(model):
    """The model's BackgroundFused (made on first use), or None when its background model is not the architecture the launch supports -- the host
    then keeps the per-op formulation."""
    f = model.__dict__.get("_bg_fused")
    if f is None:
        if not BackgroundFused.supported(model):
            return None
        f = model.__dict__["_bg_fused"] = BackgroundFused(model)
    return f


class NeRFFieldFused(_FusedState, _PrecisionGuard, _SourceWatch, _FrameLoop):
    """Caches the MFMA-ordered weight blob of a NeRFNetwork and evaluates (sigma, rgb) for sample batches."""

    def __init__(self, model):
        self.model = model
        self._init_state()
        self.precision = 1  # PNR_FIELD_F16X3 (split-fp16 matrix path, ~2^-22 relative); 0 = PNR_FIELD_FP32 (exact fmaf chains); 2 = PNR_FIELD_F16X2 (opt-in: ~1e-5 on a colour)
        self.supports_f16x2 = True
        self.table_half = False        # native loop: look the hash table up as fp16 with the reference's half interpolation (its --fp16 mode)
        m = model
        ok = (m.encoder.num_levels == 16 and m.encoder.level_dim == 2 and m.encoder.input_dim == 3 and m.hidden_dim == 64 and m.geo_feat_dim == 15
              and m.num_layers == 2 and m.num_layers_color == 3 and m.hidden_dim_color == 64 and m.encoder_dir.degree == 4)
        if not ok:
            raise RuntimeError("fused NeRF field kernel is specialised for the shipped architecture (hashgrid 16x2, 64-wide nets, SH degree 4)")

    def _weights(self):
        m = self.model
        return [_weight_of(m, "sigma_net", 0), _weight_of(m, "sigma_net", 1), _weight_of(m, "color_net", 0), _weight_of(m, "color_net", 1), _weight_of(m, "color_net", 2)]

    def _guard_tables(self):
        return [self.model.encoder.embeddings]

    def _watched(self):
        return [(w, 1) for w in self._w()] + [(self.model.encoder.embeddings, TABLE_CHECK_STRIDE)]

    def _guard_bound(self, tmax, scales):
        ws = self._weights()
        l1 = [float(v) for v in torch.stack([_l1(w).float() for w in ws]).cpu().tolist()]
        enc = tmax[0] * scales[0]
        h1 = l1[0] * enc                                   # sigma_net hidden (in prescaled units)
        geo = l1[1] * h1 / scales[0]                       # its 16 outputs, descaled
        c0 = l1[2] * max(1.6, geo)                         # colour net input = [SH (|Y| < 1.6 up to degree 4) ; geo]
        c1 = l1[3] * c0
        return max(enc, h1, geo, c0, c1)

    def _pack_build(self, prec):
        ws = [require(w.detach().contiguous(), torch.float32, "weight") for w in self._w()]
        blob = torch.empty(int(_lib.load().pnr_nerf_field_packed_bytes()) // 4, dtype=torch.float32, device=ws[0].device)
        call("pnr_nerf_field_pack", *[ptr(w) for w in ws], ptr(blob), _int(prec))
        return blob

    _frame_entry = "pnr_nerf_render_frame"

    def _frame_struct(self):
        a = _lib.NerfFrameArgs()
        return a, a

    def _frame_key(self, m, enc):
        return _pkey(enc.offsets)

    def _frame_workspace_bytes(self, lib, N):
        return lib.pnr_nerf_frame_workspace_bytes(N)

    def _frame_fill(self, args, a, m, enc):
        emb = require(enc.embeddings.detach(), torch.float32, "embeddings")
        if self.table_half:   # the reference's --fp16 tables
            emb = self._half_table(enc.embeddings)
        a.embeddings = emb.data_ptr()
        return (emb,)

    @torch.no_grad()
    def __call__(self, x, d):
        m = self.model
        x01 = ((x + m.bound) / (2 * m.bound)).contiguous()  # same two roundings as GridEncoder.forward (gridencoder/grid.py:142)
        enc = grid_encode_raw(m.encoder, x01)
        B = x.shape[0]
        sigmas = torch.empty(B, dtype=torch.float32, device=x.device)
        rgbs = torch.empty(B, 3, dtype=torch.float32, device=x.device)
        with self._held():
            call("pnr_nerf_field_forward", ptr(enc), ptr(require(d.contiguous(), torch.float32, "dirs")), ptr(self._pack()), _u32(B), ptr(sigmas),
                 ptr(rgbs), _int(self.effective_precision()), _f32(self.enc_scales()[0]), units=B)
        return sigmas, rgbs


class DensityFused(NeRFFieldFused):
    """sigma_net alone through the matrix cores (pnr_nerf_density_forward): sigma and the 15 geometry features of sample batches, no
    gradient.  Works for NeRFNetwork and PaletteNetwork (same encoder / sigma_net / color_net shapes; only the sigma_net part of the blob
    is read).  Users: the occupancy sweep (update_extra_state), density() under no_grad, PaletteNeRF training (geometry detached)."""

    def _guard_weights(self):   # only sigma_net runs here: colour-head updates (every training step) must not touch the guard or the blob (_blob_sources)
        return [_weight_of(self.model, "sigma_net", 0), _weight_of(self.model, "sigma_net", 1)]

    def _guard_bound(self, tmax, scales):
        l1 = [float(v) for v in torch.stack([_l1(w).float() for w in self._guard_weights()]).cpu().tolist()]
        enc = tmax[0] * scales[0]
        return max(enc, l1[0] * enc)

    @torch.no_grad()
    def __call__(self, x, scale=1.0, want_geo=True, enc=None):
        """enc: the encoder's raw level-major output at x when the caller has it already (the pair lookup of PaletteNeRF training)."""
        m = self.model
        if enc is None:
            x01 = ((x + m.bound) / (2 * m.bound)).contiguous()
            enc = grid_encode_raw(m.encoder, x01)
        B = x.shape[0]
        sigmas = torch.empty(B, dtype=torch.float32, device=x.device)
        geo = torch.empty(B, 15, dtype=torch.float32, device=x.device) if want_geo else None
        with self._held():
            call("pnr_nerf_density_forward", ptr(enc), ptr(self._pack()), _u32(B), ctypes.c_float(scale), ptr(sigmas), ptr(geo), _int(self.effective_precision()), _f32(self.enc_scales()[0]), units=B)
        return sigmas, geo


def density_fused(model):
    """The model's cached DensityFused (built on first use)."""
    d = getattr(model, "_density_fused", None)
    if d is None:
        d = model._density_fused = DensityFused(model)
    return d


class PaletteFieldFused(_FusedState, _PrecisionGuard, _SourceWatch, _FrameLoop):
    """Fused PaletteNeRF field + colour-basis composite (pnr_palette_field_forward).  Produces, per sample,
    sigma * density_scale, rgb and one packed aux row [direct 3 | view_dep 3 | omega nb | basis_rgb 3nb | unscaled 3nb | clip | pad]."""

    def __init__(self, model):
        self.model = model
        self._init_state()
        m = model
        ok = (m.encoder.num_levels == 16 and m.encoder.level_dim == 2 and m.hidden_dim == 64 and m.geo_feat_dim == 15 and m.num_layers == 2
              and m.num_layers_color == 3 and m.encoder_dir.degree == 4 and 1 <= m.num_basis <= _lib.MAX_BASIS and m.opt.clip_dim <= _lib.MAX_CLIP)
        if not ok:
            raise RuntimeError("fused palette field kernel is specialised for the shipped architecture")
        self.nb, self.pred_clip = int(m.num_basis), bool(m.opt.pred_clip)
        # without a clip head the reference composites clip_dim channels of zeros (palette/renderer.py:477,510): the map is zero whatever
        # happens, so those channels are left out of the packed aux row (52 -> 36 floats per sample for 4 bases) and returned as zeros
        self.clip_dim = int(m.opt.clip_dim) if self.pred_clip else 0
        self.precision = 1              # PNR_FIELD_F16X3; 0 = PNR_FIELD_FP32 (exact fmaf chains, pnr_palette_*'s fp32 matrix path); 2 = PNR_FIELD_F16X2 (opt-in)
        self.supports_f16x2 = True      # honoured by the 4-basis kernel without an edit head; the library runs every other shape as F16X3
        self.interleave_tables = True   # native loop: look both hash tables up through one interleaved copy (see _pair_table)
        # stand-alone calls (__call__ / network_forward: the dropin.fuse_field path) read the live tables by default.  True: they read the native loop's
        # interleaved copy instead (one 16-byte gather for both lookups) -- a cache keyed on torch's version counters with no checksum on this path, so
        # after a write through `.data` (torch_ema's copy_to / restore) invalidate_fused_caches(model) is REQUIRED, or the call reads the old tables
        self.stand_alone_pair = False
        self.table_half = False         # native loop: fp16 tables with the reference's half interpolation (its --fp16 mode; the clip head reads the half triple)
        self.aux_channels = int(_lib.load().pnr_palette_aux_channels(self.nb, self.clip_dim))

    def _weights(self):
        m = self.model
        ws = [_weight_of(m, *path) for path in (("sigma_net", 0), ("sigma_net", 1), ("diff_net", 0), ("diff_net", 1), ("diff_net", 2), ("color_net", 0), ("color_net", 1),
                                                ("color_net", 2), ("basis_net", 0), ("basis_net", 1), ("offsets_radiance_net",), ("omega_net", 0))]
        if self.pred_clip:
            ws += [_weight_of(m, "clip_net", 0), _weight_of(m, "clip_net", 1)]
        return ws

    def _tables(self):
        """The palette and the bias of offsets_radiance_net: packed into the blob next to the weights (the kernels read them from LDS)."""
        m = self.model
        return [m.basis_color, m.offsets_radiance_net.bias]

    def _watched(self):
        return [(w, 1) for w in self._w() + self._tables()] + [(t, TABLE_CHECK_STRIDE) for t in self._guard_tables()]

    def _guard_tables(self):
        m = self.model
        return [m.encoder.embeddings, m.encoder_palette.embeddings] + ([m.encoder_clip.embeddings] if self.pred_clip else [])

    def _guard_bound(self, tmax, scales):
        l1 = [float(v) for v in torch.stack([_l1(w).float() for w in self._weights()]).cpu().tolist()]
        s0, s1, d0, d1, d2, c0, c1, c2, b0, b1 = l1[:10]
        enc = tmax[0] * scales[0]
        h1 = s0 * enc
        geo = s1 * h1 / scales[0]
        dd0 = d0 * geo
        dd1 = d1 * dd0
        cc0 = c0 * max(1.6, geo)
        cc1 = c1 * cc0
        bin_ = max(tmax[1], 1.0) * scales[1]               # [enc_palette ; diffuse in (0,1)], prescaled together
        bb0 = b0 * bin_ / scales[1]                        # ELU output <= its input bound
        p = b1 * max(bb0, 1.0)
        sites = [enc, h1, geo, dd0, dd1, cc0, cc1, bin_, bb0, p]
        if self.pred_clip:
            ce = tmax[2] * scales[2]
            sites += [ce, l1[12] * ce]
        return max(sites)

    def _blob_sources(self):
        return self._w() + self._tables()

    def _pack_build(self, prec):
        # (the contiguous fp32 forms of the sources are not kept: the pack is enqueued on torch's current stream before they are freed, as for the other blobs)
        ws = self._w()
        lib = _lib.load()
        blob = torch.empty(int(lib.pnr_palette_field_packed_bytes(self.nb, self.clip_dim, int(self.pred_clip))), dtype=torch.uint8, device=ws[0].device)
        pw = _lib.PaletteWeights()
        srcs = [require(w.detach().contiguous(), torch.float32, "weight") for w in ws]      # (12 weights, 14 with the clip head: _weights' order)
        for name, w in zip(("sigma0", "sigma1", "diff0", "diff1", "diff2", "color0", "color1", "color2", "basis0", "basis1", "offsets_radiance", "omega", "clip0", "clip1"), srcs):
            setattr(pw, name, w.data_ptr())
        tabs = [require(t.detach().float().contiguous(), torch.float32, "palette / bias") for t in self._tables()]
        pw.basis_color, pw.or_bias = tabs[0].data_ptr(), tabs[1].data_ptr()
        pw.num_basis, pw.clip_dim, pw.pred_clip, pw.precision = self.nb, self.clip_dim, int(self.pred_clip), int(prec)
        rc = lib.pnr_palette_field_pack(ctypes.byref(pw), ctypes.c_void_p(blob.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "pnr_palette_field_pack")
        return blob

    def _edit_struct(self):
        """The model's RegionEdit / Stylizer state as a pnr_palette_edit (None when neither is set).  Rebuilt when the controllers' tensors
        change (object identity / version): a few small D2H copies per change, none per frame."""
        edit, sty = getattr(self.model, "edit", None), getattr(self.model, "stylizer", None)
        if edit is None and sty is None:
            return None
        if sty is not None:
            key = ("s", id(sty), _pkey(sty.dI), _pkey(sty.dP), _pkey(sty.ddelta))
        else:
            key = ("e", id(edit), float(edit.std_xyz), float(edit.std_clip), bool(edit.weight_mode)) + tuple(
                _pkey(t) if torch.is_tensor(t) else None for t in (edit.delta_hsv, edit.mean_xyz, edit.mean_clip))
        return self._cache.get("edit", key, self._edit_build, edit, sty)

    def _edit_build(self, edit, sty):
        e = _lib.PaletteEdit()
        nb = self.nb
        if sty is not None:    # palette/renderer.py:150-183
            e.mode = 2
            dI, dP, dd = sty.dI.detach().float().cpu(), sty.dP.detach().float().cpu().reshape(nb, 3), sty.ddelta.detach().float().cpu()
            for b in range(nb):
                e.dI[b] = float(dI[b])
                for k in range(3):
                    e.dP[b][k] = float(dP[b, k])
                    for j in range(3):
                        e.ddelta[b][k][j] = float(dd[b, k, j])
        else:                  # palette/renderer.py:84-147
            e.mode = 1
            dh = edit.delta_hsv.detach().float().cpu()
            for b in range(nb):
                for k in range(3):
                    e.delta_hsv[b][k] = float(dh[b, k])
            if edit.mean_xyz is not None:
                e.has_mean_xyz = 1
                for k, v in enumerate(edit.mean_xyz.detach().float().cpu().reshape(-1)[:3].tolist()):
                    e.mean_xyz[k] = v
            if edit.mean_clip is not None:
                mc = edit.mean_clip.detach().float().cpu().reshape(-1).tolist()
                if len(mc) != int(self.model.opt.clip_dim):
                    raise RuntimeError("RegionEdit.mean_clip must have clip_dim entries")
                e.has_mean_clip = len(mc)
                for k, v in enumerate(mc):
                    e.mean_clip[k] = v
            e.std_xyz, e.std_clip, e.weight_mode = float(edit.std_xyz), float(edit.std_clip), int(bool(edit.weight_mode))
        return e

    @torch.no_grad()
    def _interleaved(self, slot, encs, build):
        ts = [e.embeddings for e in encs]
        if any(t.dtype != torch.float32 or t.shape != ts[0].shape or t.shape[1] != 2 for t in ts):
            return None
        half = bool(self.table_half)
        return self._cache.get(slot, tuple(_pkey(t) for t in ts) + (half,), build, [t.detach() for t in ts], half)

    def _pair_table(self):
        """`encoder` and `encoder_palette` interleaved row by row ([rows, 4] fp32; one 16-byte gather then serves both lookups; table_half: rows of 4
        halves).  A copy of both tables (2 x 50 MB for the shipped config): ONE slot with table_half in its key, so that it is never held twice."""
        return self._interleaved("pair", (self.model.encoder, self.model.encoder_palette), self._pair_build)

    def _pair_build(self, ts, half):
        a, b = ts
        if half:   # rows of 4 halves: (a.x, a.y, b.x, b.y)
            return torch.cat([a.to(torch.float16), b.to(torch.float16)], dim=1).contiguous()
        out = torch.empty(a.shape[0], 4, dtype=torch.float32, device=a.device)
        call("pnr_interleave_tables", ptr(a.contiguous()), ptr(b.contiguous()), ctypes.c_uint64(a.shape[0]), ptr(out))
        return out

    def _triple_table(self):
        """--pred_clip: the three tables interleaved row by row ([rows, 8] fp32 = encoder, encoder_palette, encoder_clip, 2 pad): one 32-byte
        row per corner serves all three lookups.  table_half: [rows, 8] fp16 instead (one 16-byte row).  A slot each: ("triple", half)."""
        m = self.model
        return self._interleaved(("triple", bool(self.table_half)), (m.encoder, m.encoder_palette, m.encoder_clip), self._triple_build)

    def _triple_build(self, ts, half):
        out = torch.empty(ts[0].shape[0], 8, dtype=torch.float16 if half else torch.float32, device=ts[0].device)
        call("pnr_interleave_tables3_half" if half else "pnr_interleave_tables3", *[ptr(t.contiguous()) for t in ts], ctypes.c_uint64(ts[0].shape[0]), ptr(out))
        return out

    _frame_entry = "pnr_palette_render_frame"
    _frame_finish_mask = 7

    def _frame_struct(self):
        p = _lib.PaletteFrameArgs()
        return p, p.base

    def _frame_key(self, m, enc):
        return (bool(self.interleave_tables), float(m.offsets_weight), float(m.view_dep_weight),
                tuple((_pkey(o.offsets), o.per_level_scale) for o in (enc, m.encoder_palette, m.encoder_clip)))

    def _frame_workspace_bytes(self, lib, N):
        return lib.pnr_palette_frame_workspace_bytes(N, self.nb, self.clip_dim, int(self.pred_clip))

    def _frame_fill(self, p, a, m, enc):
        # (once per set of offset buffers: torch.equal is a device comparison plus a host read)
        for other in (m.encoder_palette, m.encoder_clip):
            if not torch.equal(other.offsets, enc.offsets) or other.per_level_scale != enc.per_level_scale:
                raise RuntimeError("the three hash grids must share one level layout")
        a.embeddings = require(enc.embeddings.detach(), torch.float32, "embeddings").data_ptr()
        p.embeddings_palette = require(m.encoder_palette.embeddings.detach(), torch.float32, "embeddings").data_ptr()
        p.embeddings_clip = require(m.encoder_clip.embeddings.detach(), torch.float32, "embeddings").data_ptr() if self.pred_clip else None
        p.num_basis, p.clip_dim, p.pred_clip = self.nb, self.clip_dim, int(self.pred_clip)
        p.offsets_weight, p.view_dep_weight = float(m.offsets_weight), float(m.view_dep_weight)
        pair = self._pair_table() if ((self.interleave_tables or self.table_half) and not self.pred_clip) else None
        p.embeddings_pair = pair.data_ptr() if pair is not None else None
        triple = self._triple_table() if ((self.interleave_tables or self.table_half) and self.pred_clip) else None
        p.embeddings_triple = triple.data_ptr() if triple is not None else None
        return pair, triple

    def _frame_extras(self, tok, N, dev):
        p, a, finished = tok.args, tok.base, tok.finished
        aux_map = torch.empty(N, self.aux_channels, dtype=torch.float32, device=dev)
        tok.out += (aux_map,)
        p.aux_map = aux_map.data_ptr()
        tok.depth_raw = torch.empty(N, dtype=torch.float32, device=dev) if finished else None
        a.depth_raw = tok.depth_raw.data_ptr() if finished else None
        edit = tok.edit = self._edit_struct()
        p.edit = ctypes.cast(ctypes.pointer(edit), ctypes.c_void_p) if edit is not None else None

    def _frame_outputs(self, tok, stats):
        stats["depth_raw"] = tok.depth_raw
        return tok.out + (stats,)

    @torch.no_grad()
    def network_forward(self, x, d):
        """PaletteNetwork.forward(x, d) (palette/network.py:156-190) as ONE launch behind the lookups: returns what the reference's method returns --
        (sigma [B] unscaled, clip_feat [B, clip_dim], omega [B, nb] normalised, offsets_radiance [B, 3 nb + 1], view_dep [B, 3], diffuse [B, 3]) --
        the last five as slices of one packed row (pnr_palette_edit.mode 3).  Inference only (no autograd graph)."""
        heads = _lib.PaletteEdit()
        heads.mode = 3
        sigmas, _, row = self(x, d, _edit=heads, _density_scale=1.0)
        nb, cd = self.nb, int(self.model.opt.clip_dim)
        omega = row[:, :nb]
        offsets_radiance = row[:, nb:4 * nb + 1]
        view_dep = row[:, 4 * nb + 1:4 * nb + 4]
        diffuse = row[:, 4 * nb + 4:4 * nb + 7]
        clip_feat = row[:, 4 * nb + 7:4 * nb + 7 + cd] if self.pred_clip else sigmas.new_zeros(sigmas.shape[0], cd)    # palette/network.py:179
        return sigmas, clip_feat, omega, offsets_radiance, view_dep, diffuse

    def __call__(self, x, d, deltas=None, _edit=None, _density_scale=None):
        """x [B,3] world positions, d [B,3] -> (sigmas [B] scaled by density_scale, rgbs [B,3], aux [B, aux_channels])."""
        m = self.model
        lib = _lib.load()
        B = x.shape[0]
        dev = x.device
        x01 = ((x + m.bound) / (2 * m.bound)).contiguous()
        pair = None
        if self.stand_alone_pair and self.interleave_tables and not self.pred_clip and not self.table_half and pairable(m.encoder, m.encoder_palette):
            pair = self._pair_table()       # opt-in (stand_alone_pair): the native loop's interleaved copy, rebuilt when torch can tell either table changed
        if pair is not None:
            enc, enc_pal = _encode_pair(m.encoder, pair, x01)
        else:
            enc = grid_encode_raw(m.encoder, x01)
            enc_pal = grid_encode_raw(m.encoder_palette, x01)
        enc_clip = grid_encode_raw(m.encoder_clip, x01) if self.pred_clip else None
        sigmas = torch.empty(B, dtype=torch.float32, device=dev)
        rgbs = torch.empty(B, 3, dtype=torch.float32, device=dev)
        aux = torch.empty(B, self.aux_channels, dtype=torch.float32, device=dev)
        a = _lib.PaletteFieldArgs()
        a.ctl, a.B = None, B
        a.enc, a.enc_palette = enc.data_ptr(), enc_pal.data_ptr()
        a.enc_clip = enc_clip.data_ptr() if enc_clip is not None else None
        a.level_stride = B
        a.dirs = require(d.contiguous(), torch.float32, "dirs").data_ptr()
        a.deltas = deltas.data_ptr() if deltas is not None else None
        a.packed = self._pack().data_ptr()
        a.num_basis, a.clip_dim, a.pred_clip = self.nb, self.clip_dim, int(self.pred_clip)
        a.density_scale, a.offsets_weight, a.view_dep_weight = float(m.density_scale if _density_scale is None else _density_scale), float(m.offsets_weight), float(m.view_dep_weight)
        a.aux_stride = self.aux_channels
        a.sigmas, a.rgbs, a.aux = sigmas.data_ptr(), rgbs.data_ptr(), aux.data_ptr()
        a.precision = int(self.effective_precision())
        if _edit is not None and a.precision == 2:
            a.precision = 1          # (the rounded-activation form exists for the composite kernels only)
        for k, v in enumerate(self.enc_scales()):
            a.enc_scale[k] = v
        edit = self._edit_struct() if _edit is None else _edit
        a.edit = ctypes.cast(ctypes.pointer(edit), ctypes.c_void_p) if edit is not None else None
        xw = require(x.contiguous(), torch.float32, "xyzs")
        a.xyzs = xw.data_ptr()
        rc = lib.pnr_palette_field_forward(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "pnr_palette_field_forward")
        return sigmas, rgbs, aux
