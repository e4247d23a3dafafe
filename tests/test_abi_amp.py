"""The loss-scaled optimiser step's C entries (pnr_grad_check, pnr_adam_step_amp) and its host side, without a device: symbols, argument
validation, the scalar rows the host forms, and the scaler's state_dict."""
import ctypes

import numpy as np


def test_symbols_resolve_and_the_abi_version_is_unchanged():
    from palettenerf_amd import _lib
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    for name in ("pnr_grad_check", "pnr_adam_step_amp"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.AdamAmpCtl) == 32 and _lib.AdamAmpCtl.skipped_base.offset == 24 and _lib.AdamAmpCtl.parity.offset == 28


def test_argument_validation_without_gpu():
    from palettenerf_amd import _lib
    lib = _lib.load()
    u32 = ctypes.c_uint32
    cap = int(lib.pnr_adam_max_tensors())
    INVALID, UNSUPPORTED = -1, -2
    some = ctypes.c_void_p(0x1000)          # never dereferenced: every case below returns before a launch
    one = (_lib.AdamTensor * 1)()
    many = (_lib.AdamTensor * (cap + 1))()
    rows = (_lib.AdamScalars * 8)()
    ctl = _lib.AdamAmpCtl()
    ctl.scale = ctl.found_inf = ctl.state = 0x1000

    assert lib.pnr_grad_check(None, u32(0), None, None) == 0                       # nothing to check
    assert lib.pnr_grad_check(None, u32(1), some, None) == INVALID
    assert lib.pnr_grad_check(one, u32(1), None, None) == INVALID
    assert lib.pnr_grad_check(many, u32(cap + 1), some, None) == UNSUPPORTED
    assert lib.pnr_grad_check(one, u32(1), some, None) == 0                        # n == 0 tensors are skipped: no launch
    one[0].n = 4
    assert lib.pnr_grad_check(one, u32(1), some, None) == INVALID                  # n > 0 and no gradient pointer
    one[0].n = 0

    assert lib.pnr_adam_step_amp(None, u32(0), None, u32(0), None, None) == 0
    assert lib.pnr_adam_step_amp(None, u32(1), rows, u32(8), ctypes.byref(ctl), None) == INVALID
    assert lib.pnr_adam_step_amp(one, u32(1), None, u32(8), ctypes.byref(ctl), None) == INVALID
    assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(8), None, None) == INVALID
    for field in ("scale", "found_inf", "state"):
        bad = _lib.AdamAmpCtl()
        bad.scale = bad.found_inf = bad.state = 0x1000
        setattr(bad, field, None)
        assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(8), ctypes.byref(bad), None) == INVALID, field
    assert lib.pnr_adam_step_amp(many, u32(cap + 1), rows, u32(8), ctypes.byref(ctl), None) == UNSUPPORTED
    assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(0), ctypes.byref(ctl), None) == UNSUPPORTED
    assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(9), ctypes.byref(ctl), None) == UNSUPPORTED
    assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(8), ctypes.byref(ctl), None) == 0     # n == 0: skipped, no launch
    one[0].n = 4
    assert lib.pnr_adam_step_amp(one, u32(1), rows, u32(8), ctypes.byref(ctl), None) == INVALID


def torch_scalars(lr, beta1, beta2, eps, step):
    """torch/optim/adam.py's host scalars (Python doubles), narrowed to fp32 as pnr_adam_scalars holds them."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    f = lambda x: float(np.float32(x))
    return dict(one_minus_beta1=f(1 - beta1), beta2=f(beta2), one_minus_beta2=f(1 - beta2), bias_correction2_sqrt=f(bias_correction2 ** 0.5),
                eps=f(eps), neg_step_size=f(-(lr / bias_correction1)), inv_grad_scale=1.0)


def test_the_rows_are_the_plain_steps_scalars_for_the_lower_step_counts():
    from palettenerf_amd import _lib, optim
    hyper = (1e-2, 0.9, 0.99, 1e-15)
    fields = [name for name, _ in _lib.AdamScalars._fields_]
    for calls, skipped_base in ((1, 0), (3, 0), (8, 0), (9, 1), (40, 13), (1000, 7)):
        step = calls - skipped_base                               # the optimistic count: every call the host has not seen skipped was taken
        rows, n_rows = optim.Adam._amp_rows(*hyper, step)
        assert len(rows) == 8 and n_rows == min(8, step)          # a step count below 1 has no row
        for r in range(n_rows):
            plain = optim.Adam._scalars(*hyper, calls - skipped_base - r)
            want = torch_scalars(*hyper, calls - skipped_base - r)
            for name in fields:
                assert getattr(rows[r], name) == getattr(plain, name) == want[name], (calls, skipped_base, r, name)


def test_scaler_state_dict_keys_are_torchs(monkeypatch):
    import torch
    from palettenerf_amd import optim
    # (without a device torch would disable both scalers and hand out two empty dicts; before the first scale() neither touches a device)
    monkeypatch.setattr(torch.cuda.amp.common, "amp_definitely_not_available", lambda: False)
    kw = dict(init_scale=2.0 ** 15, growth_interval=2)
    ours, theirs = optim.GradScaler("cuda", **kw), torch.amp.GradScaler("cuda", **kw)
    assert issubclass(optim.GradScaler, torch.amp.GradScaler) and ours.is_enabled() and theirs.is_enabled()
    assert ours.state_dict() == theirs.state_dict() and ours.state_dict()["scale"] == 2.0 ** 15 and len(ours.state_dict()) == 5
    assert ours.state_dict().keys() == theirs.state_dict().keys()
    for name in ("scale", "update", "get_scale", "state_dict", "load_state_dict", "unscale_"):
        assert getattr(optim.GradScaler, name) is getattr(torch.amp.GradScaler, name), name
