"""Guard bands around the arrays of a C-ABI call: did a launch write a byte outside its outputs or its workspace, and does a result depend on a
byte outside its inputs?

Every array of a guarded call is a view into a uint8 buffer with at least GUARD bytes in front of it and at least GUARD bytes behind it; the
back guard begins at the byte after the view's last element.  Around an output and a workspace the guard is one sentinel byte; around a floating
input it is all-ones bytes (a NaN in fp32 and in fp16: a value read from there poisons the result); around an integer array that a kernel uses as
an index or a count the caller names values that are valid for the array's meaning, so that using them changes an output but never indexes
outside an allocation.  Plain torch: works on CPU tensors too (tests/test_guard_bands_host.py tests it there)."""
import torch

GUARD = 64 * 1024        # a runaway 128 x 64 fp32 tile is 32 KiB
SENTINEL = 0xA5          # around outputs and workspaces
NAN_BYTE = 0xFF          # around floating inputs: 0xFFFFFFFF / 0xFFFF are NaNs

last_report = ""         # what the last failing untouched() saw


def _buffer(nbytes, device, align, fill):
    """uint8 buffer of GUARD + nbytes + GUARD (+ slack for the alignment) bytes, every byte `fill`; -> (buffer, offset of the view in it) with
    (address of the view) % 256 == align % 256."""
    buf = torch.full((2 * GUARD + 512 + nbytes,), fill, dtype=torch.uint8, device=device)
    start = GUARD + (align - (buf.data_ptr() + GUARD)) % 256
    return buf, start


def _view(buf, start, shape, dtype):
    nbytes = _nbytes(shape, dtype)
    flat = buf[start:start + nbytes]
    if dtype != torch.uint8:
        flat = flat.view(dtype)
    return flat.view(shape)


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _nbytes(shape, dtype):
    n = 1
    for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(s)
    return n * _itemsize(dtype)


def _finish(buf, start, nbytes, expected):
    buf._guard = (start, nbytes, expected)      # expected: an int (every guard byte) or a uint8 tensor, the buffer as it was built
    return buf


def out(shape, dtype, device, align=256, fill=SENTINEL):
    """(buffer, view): a contiguous `shape` view of `dtype` inside a sentinel-filled buffer.  The view itself holds sentinel bytes too: fill it as
    the entry's caller would."""
    shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
    assert align % _itemsize(dtype) == 0, "a view cannot start inside one of its own elements"
    nbytes = _nbytes(shape, dtype)
    buf, start = _buffer(nbytes, device, align, fill)
    view = _view(buf, start, shape, dtype)
    assert (nbytes == 0 or view.data_ptr() % 256 == align % 256) and view.is_contiguous()      # (an empty view has no address)
    return _finish(buf, start, nbytes, fill), view


def workspace(nbytes, device, align=256):
    """(buffer, view): a guarded uint8 region of exactly `nbytes` bytes -- what the entry's *_workspace_bytes function returned, not rounded up."""
    return out((int(nbytes),), torch.uint8, device, align)


def inp(tensor, align=256, around=None):
    """(buffer, view): a guarded copy of `tensor`.  around: None for a floating array (all-ones bytes, NaN); for an integer array either a sequence
    of element values valid for the array's meaning, tiled so that whole copies end at the view's first byte and begin at the byte after its last
    -- e.g. the ray triple (0, 0, 1), a live ray id, the last offset -- or, for integers that are data and not indices (a bitfield), an int byte."""
    t = tensor.contiguous()
    if around is None:
        if not t.dtype.is_floating_point:
            raise ValueError("an integer array needs `around`: values valid for its meaning (never a bit pattern around an index array)")
        around = NAN_BYTE
    if isinstance(around, int):
        buf, start = _buffer(t.numel() * t.element_size(), t.device, align, around)
        expected = around
    else:
        pattern = torch.tensor(list(around), dtype=t.dtype).contiguous().view(torch.uint8).to(t.device)
        buf, start = _buffer(t.numel() * t.element_size(), t.device, align, 0)
        p, nbytes = pattern.numel(), t.numel() * t.element_size()
        front = pattern.repeat(start // p + 2)
        buf[:start] = front[front.numel() - start:]
        back = buf.numel() - start - nbytes
        buf[start + nbytes:] = pattern.repeat(back // p + 1)[:back]
        expected = None
    assert align % t.element_size() == 0, "a view cannot start inside one of its own elements"
    view = _view(buf, start, tuple(t.shape), t.dtype)
    view.copy_(t)
    assert t.numel() == 0 or view.data_ptr() % 256 == align % 256
    return _finish(buf, start, t.numel() * t.element_size(), buf.clone() if expected is None else expected), view


def untouched(buffer, view=None):
    """True when every guard byte of `buffer` is what it was built with.  When False, `last_report` names the first
    touched byte by its offset relative to the view: negative in front of it, >= the view's size behind it."""
    global last_report
    start, nbytes, expected = buffer._guard
    if view is not None and view.numel() > 0:       # (an empty view has no address)
        assert view.data_ptr() == buffer.data_ptr() + start, "not the view of this buffer"
    end = start + nbytes
    if isinstance(expected, int):
        bad_front, bad_back = buffer[:start] != expected, buffer[end:] != expected
    else:
        bad_front, bad_back = buffer[:start] != expected[:start], buffer[end:] != expected[end:]
    if not bool(bad_front.any() | bad_back.any()):
        return True
    if bool(bad_front.any()):
        first = int(torch.nonzero(bad_front)[0]) - start
        n_front = int(bad_front.sum())
        last_report = f"first touched byte {-first} bytes in front of the view (offset {first}); {n_front} guard bytes in front differ"
    else:
        first = int(torch.nonzero(bad_back)[0])
        last_report = (f"first touched byte {first} bytes behind the end (offset {nbytes + first} from the view's start); "
                       f"{int(bad_back.sum())} guard bytes behind differ")
    return False


def first_touched(buffer):
    """Offset of the first touched guard byte relative to the view's first byte (None: untouched)."""
    start, nbytes, expected = buffer._guard
    diff = buffer != expected
    diff[start:start + nbytes] = False
    idx = torch.nonzero(diff)
    return None if idx.numel() == 0 else int(idx[0]) - start
