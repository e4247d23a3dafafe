"""The weights' average without a device: the C entries (pnr_ema_update, pnr_ema_swap) -- symbols, the struct's layout, every validation
code -- and the host side of optim.ExponentialMovingAverage: the decay doubles, torch_ema's state_dict format,
and that nothing falls back to the CPU.  The control is tests/ema_reference.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ema_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("pnr_ema_update", "pnr_ema_swap")


def test_symbols_resolve_and_the_abi_version_is_unchanged():
    from palettenerf_amd import _lib
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    for name in ENTRIES:
        assert f"int {name}(" in hdr, name
    assert ctypes.sizeof(_lib.AdamTensor) == 40                      # the step's tensor struct did not grow


def test_the_ctypes_mirror_has_the_layout_gcc_gives_pnr_ema_tensor(tmp_path):
    from palettenerf_amd import _lib
    fields = [f[0] for f in _lib.EmaTensor._fields_]
    assert fields == ["param", "shadow", "n"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(pnr_ema_tensor));']
    lines += [f'  printf("{f} %zu\\n", offsetof(pnr_ema_tensor, {f}));' for f in fields]
    lines += ['  pnr_ema_tensor t = {0, 0, 0}; (void)t;', '  return 0;', '}']      # (three members: a fourth in the header would warn, a third missing fails)
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.EmaTensor) == 24
    for f in fields:
        assert int(got[f]) == getattr(_lib.EmaTensor, f).offset, f


def test_argument_validation_without_gpu():
    from palettenerf_amd import _lib
    lib = _lib.load()
    u32, f32 = ctypes.c_uint32, ctypes.c_float
    cap = int(lib.pnr_adam_max_tensors())
    OK, INVALID, UNSUPPORTED = 0, -1, -2
    w = f32(0.05)
    # (no pointer below is ever dereferenced on the device: every case returns before a launch)
    for call in (lambda arr, n: lib.pnr_ema_update(arr, u32(n), w, None), lambda arr, n: lib.pnr_ema_swap(arr, u32(n), None)):
        one = (_lib.EmaTensor * 1)()
        many = (_lib.EmaTensor * (cap + 1))()
        assert call(None, 0) == OK                                      # nothing to do
        assert call(None, 1) == INVALID                                 # no array
        assert call(many, cap + 1) == UNSUPPORTED
        assert call(one, 1) == OK                                       # n == 0 tensors are skipped: no launch
        one[0].n = 4
        assert call(one, 1) == INVALID                                  # n > 0, neither pointer
        one[0].param = 0x1000
        assert call(one, 1) == INVALID                                  # ... no shadow
        one[0].param, one[0].shadow = None, 0x1000
        assert call(one, 1) == INVALID                                  # ... no parameter


@pytest.mark.parametrize("decay,switch", [(0.95, 170), (0.5, 8)])
def test_the_decay_doubles_are_torch_emas(decay, switch):
    """min(decay, (1 + k) / (10 + k)) in Python doubles for k = 1 .. 200: the warm-up below the switch, `decay` above it, and at the switch
    whichever double is smaller ((1 + k) / (10 + k) == decay in exact arithmetic there).  The weight the kernels get is the fp32 narrowing of
    the double 1.0 - decay_k."""
    from palettenerf_amd import optim
    for k in range(1, 201):
        got = optim.ExponentialMovingAverage.decay_at(decay, k)
        assert got == ref.decay_at(decay, k), k
        warm = (1 + k) / (10 + k)
        if k < switch:
            assert got == warm < decay, k
        elif k > switch:
            assert got == decay < warm, k
        else:
            assert got == min(decay, warm) and abs(warm - decay) < 1e-15, k
        assert ctypes.c_float(1.0 - got).value == float(np.float32(1.0 - got)), k


def cpu_parameters():
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 1, 0, 7)]
    ps[1].requires_grad_(False)                                       # a frozen one is tracked as well (torch_ema 0.3)
    return ps


def test_state_dict_round_trip_on_cpu_tensors():
    from palettenerf_amd import optim
    ps = cpu_parameters()
    ema = optim.ExponentialMovingAverage(ps, 0.95)
    assert len(ema.shadow_params) == 4 and ema.collected_params is None and ema.decay == 0.95 and ema.num_updates == 0
    assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() and not s.requires_grad for s, p in zip(ema.shadow_params, ps) if p.numel())
    sd = ema.state_dict()
    assert list(sd) == list(ref.ControlEMA(ps, 0.95).state_dict()) == ["decay", "num_updates", "shadow_params", "collected_params"]
    with torch.no_grad():
        for p in ps:
            p.mul_(2.0)
    ema.store()
    sd = ema.state_dict()
    other = optim.ExponentialMovingAverage(cpu_parameters(), 0.5)
    other.load_state_dict(sd)
    assert other.decay == 0.95 and other.num_updates == 0
    assert all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    assert all(torch.equal(a, b) for a, b in zip(other.collected_params, ema.collected_params))
    assert other.shadow_params[0].data_ptr() != ema.shadow_params[0].data_ptr()        # its own copies
    # store / copy_to / restore keep torch_ema's meaning, and move the version of every parameter they write
    versions = [p._version for p in ps]
    ema.copy_to()
    assert all(torch.equal(p, s) for p, s in zip(ps, ema.shadow_params)) and all(p._version > v for p, v in zip(ps, versions))
    versions = [p._version for p in ps]
    ema.restore()
    assert all(torch.equal(p, c) for p, c in zip(ps, ema.collected_params)) and all(p._version > v for p, v in zip(ps, versions))
    with pytest.raises(ValueError):
        optim.ExponentialMovingAverage(ps[:2], 0.95).load_state_dict(sd)                 # the wrong number of parameters
    with pytest.raises(ValueError):
        optim.ExponentialMovingAverage(ps, 1.5)


def test_a_hand_built_torch_ema_state_dict_loads():
    """What a reference checkpoint's 'ema' entry holds (palette/utils.py:1221-1222: torch_ema's state_dict), double shadows included: cast to
    the parameters' dtype as torch_ema does."""
    from palettenerf_amd import optim
    ps = cpu_parameters()
    shadows = [torch.full((p.numel(),), float(i + 1), dtype=torch.float64) for i, p in enumerate(ps)]
    sd = {"decay": 0.95, "num_updates": 1234, "shadow_params": shadows, "collected_params": None}
    ema = optim.ExponentialMovingAverage(ps, 0.9)
    ema.load_state_dict(sd)
    assert ema.decay == 0.95 and ema.num_updates == 1234 and ema.collected_params is None
    assert all(s.dtype == torch.float32 and torch.equal(s, want.float()) for s, want in zip(ema.shadow_params, shadows))
    assert shadows[0].dtype == torch.float64                          # the caller's dict is not touched
    for broken in ({**sd, "num_updates": 1.5}, {**sd, "shadow_params": tuple(shadows)}, {**sd, "collected_params": shadows[:1]}, {**sd, "decay": -0.1}):
        with pytest.raises(ValueError):
            optim.ExponentialMovingAverage(ps, 0.9).load_state_dict(broken)


def test_update_and_swap_on_cpu_tensors_raise_and_touch_nothing():
    from palettenerf_amd import optim
    ps = cpu_parameters()
    ema = optim.ExponentialMovingAverage(ps, 0.95)
    with torch.no_grad():
        ps[0].add_(1.0)
    before = [p.detach().clone() for p in ps], [s.clone() for s in ema.shadow_params]
    for call in (ema.update, ema.swap):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with ema.average_parameters():
            pass
    assert ema.num_updates == 0
    assert all(torch.equal(p, b) for p, b in zip(ps, before[0])) and all(torch.equal(s, b) for s, b in zip(ema.shadow_params, before[1]))
