"""The training path's optimiser step as one HIP launch: `Adam` is a drop-in for `torch.optim.Adam` as the reference constructs it
(main_nerf.py:113, main_palette.py:223: lr 1e-2, betas (0.9, 0.99), eps 1e-15) -- same constructor, param groups, state_dict keys
(`step`, `exp_avg`, `exp_avg_sq`) and, bit for bit, the same updates (pnr_adam_step) -- so schedulers, GradScaler and checkpoints of the
reference's trainer work unchanged.  torch runs seven elementwise kernels per parameter tensor (~75 launches and seven passes over the
50 MB hash tables per step); this makes one pass in one launch.

`GradScaler` is `torch.amp.GradScaler` for the reference's default `-O` recipe (fp16 autocast + loss scaling) whose `step` stays on the device
with `Adam`: a finite check that writes one flag (pnr_grad_check) and the step under that flag (pnr_adam_step_amp) instead of torch's
`unscale_` pass and its `found_inf.item()` read-back per training step -- torch's bits, skipped steps included.

`ExponentialMovingAverage` is torch_ema's, which every recipe of the reference keeps over the model's parameters: `update` as one launch
(pnr_ema_update) and `swap` (pnr_ema_swap) in place of store + copy_to / restore around an evaluation -- torch_ema's bits and state_dict.
"""
import contextlib
import copy
import ctypes
import weakref

import numpy as np
import torch
from torch.amp.grad_scaler import OptState

from . import _lib


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise ValueError("palettenerf_amd.optim.Adam covers the reference's configuration: no weight decay, no amsgrad")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))
        self.grad_scale = None   # set to GradScaler's scale (a float) to fold unscale_ into the step; None / 1.0 = gradients as they are

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        cap = int(lib.pnr_adam_max_tensors())
        self._amp_reconcile()   # (steps enqueued through GradScaler.step, below: their skips come off `step` first)
        # ONE launch for every tensor that shares its hyperparameters and step count (the reference's get_params makes ten param groups with the
        # same lr / betas / eps: torch runs them group by group); tensors that joined later have their own bias corrections and go separately
        batches = {}
        todo = []
        for group in self.param_groups:      # first pass: every check, nothing touched -- a rejected tensor must not leave earlier ones a step ahead
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("palettenerf_amd.optim.Adam: dense fp32 CUDA(HIP) parameters only (no CPU fallback)")
                if not (p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("palettenerf_amd.optim.Adam: parameters and gradients must be contiguous")
                todo.append((group, p))
        for group, p in todo:
            beta1, beta2 = group["betas"]
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)   # host tensor, as torch keeps it for non-capturable Adam
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            key = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), int(st["step"].item()), p.device.index)
            batches.setdefault(key, []).append((p, st))
        for (lr, beta1, beta2, eps, step, _dev), items in batches.items():
            sc = self._scalars(lr, beta1, beta2, eps, step, self.grad_scale)
            for i in range(0, len(items), cap):
                arr = self._tensor_array(items[i:i + cap])
                with torch.cuda.device(_dev):   # the launch goes to the tensors' device, on torch's current stream there
                    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    _lib.check(lib.pnr_adam_step(arr, ctypes.c_uint32(len(arr)), ctypes.byref(sc), stream), "pnr_adam_step")
            for p, _ in items:
                torch.autograd.graph.increment_version(p)   # written by a raw kernel: caches keyed on the version (packed blobs, pair tables) must see it
        return loss

    @staticmethod
    def _scalars(lr, beta1, beta2, eps, step, grad_scale=None):
        """The host scalars exactly as torch/optim/adam.py forms them (Python floats), narrowed where its CUDA kernels narrow them."""
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        sc = _lib.AdamScalars()
        sc.one_minus_beta1, sc.beta2, sc.one_minus_beta2 = 1 - beta1, beta2, 1 - beta2
        sc.bias_correction2_sqrt = bias_correction2_sqrt
        sc.eps, sc.neg_step_size = eps, -step_size
        sc.inv_grad_scale = 1.0 if not grad_scale else float(np.float32(1.0) / np.float32(grad_scale))
        return sc

    @staticmethod
    def _tensor_array(items):
        arr = (_lib.AdamTensor * len(items))()
        for k, (p, st) in enumerate(items):
            arr[k].param, arr[k].grad = p.data_ptr(), p.grad.data_ptr()
            arr[k].exp_avg, arr[k].exp_avg_sq, arr[k].n = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
        return arr

    # ---------------------------------------------------------------- the loss-scaled (-O) step: GradScaler.step without a read-back
    #
    # torch's GradScaler.step reads found_inf back on every step to decide whether to call optimizer.step().  Here the decision is the device's
    # (pnr_adam_step_amp), and what the host does not know -- how many of the steps it has enqueued were skipped -- it bounds: `step` advances
    # optimistically, the device's count of skipped steps follows every step into pinned memory behind an event, and the launch carries the
    # scalars of the step for 0 .. AMP_ROWS - 1 skips the host has not seen yet (the device picks the row).  Skips the host learns of are taken
    # off every `step`; it waits only if the oldest step it has not seen the end of is AMP_ROWS calls back.
    AMP_ROWS = 8

    @classmethod
    def _amp_rows(cls, lr, beta1, beta2, eps, step):
        """(rows, n_rows): row r = the scalars of true step count `step - r` (`step` = the optimistic count: every enqueued step taken); a step
        count below 1 cannot be (no more steps were skipped than made), so n_rows = min(AMP_ROWS, step)."""
        n_rows = max(1, min(cls.AMP_ROWS, int(step)))
        rows = (_lib.AdamScalars * cls.AMP_ROWS)()
        for r in range(n_rows):
            rows[r] = cls._scalars(lr, beta1, beta2, eps, step - r)
        return rows, n_rows

    def _amp_init(self, device):
        amp = self.__dict__.get("_amp")
        if amp is None or amp["device"] != device:
            if amp is not None:
                self._amp_reconcile()
            amp = self.__dict__["_amp"] = dict(
                device=device,
                found_inf=torch.zeros((), dtype=torch.float32, device=device),
                state=torch.zeros(3, dtype=torch.int32, device=device),          # {skipped, skipped, error}: pnr_adam_amp_ctl.state
                pinned=torch.zeros(2 * self.AMP_ROWS, 3, dtype=torch.int32).pin_memory(),
                calls=0,              # amp steps launched: the ping-pong parity and the pinned slot
                skipped_base=0,       # skipped steps the host has seen (and taken off every `step`)
                pending=[],           # (event, slot, parity after the step) of the steps whose end the host has not seen, oldest first
                params=[])            # the parameters of the pending steps (the same set for all of them)
        return amp

    def _amp_observe(self, slot, parity):
        amp = self._amp
        row = amp["pinned"][slot]
        if int(row[2]) != 0:
            raise RuntimeError("palettenerf_amd.optim.Adam: the device found no scalar row for a loss-scaled step (more skipped steps than rows)")
        new = int(row[parity]) - amp["skipped_base"]
        if new:
            for p in amp["params"]:
                self.state[p]["step"] -= new
            amp["skipped_base"] += new

    def _amp_poll(self, keep):
        """Take in every finished step's count of skips, oldest first; wait until at most `keep` steps are unobserved."""
        amp = self.__dict__.get("_amp")
        if amp is None:
            return
        pending = amp["pending"]
        while pending:
            event, slot, parity = pending[0]
            if not event.query():
                if len(pending) <= keep:
                    break
                event.synchronize()
            pending.pop(0)
            if not pending or not pending[0][0].query():       # the newest finished one carries every earlier skip
                self._amp_observe(slot, parity)

    def _amp_reconcile(self):
        """Every enqueued loss-scaled step observed (waits for the device): `step` is then the true count, as torch keeps it."""
        self._amp_poll(0)

    def state_dict(self):
        self._amp_reconcile()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._amp_reconcile()
        return super().load_state_dict(state_dict)

    @torch.no_grad()
    def _amp_step(self, scale):
        """GradScaler.step's device path (called by palettenerf_amd.optim.GradScaler): the finite check over every gradient, then the step under
        the flag.  Returns the flag (a device fp32 scalar: GradScaler.update's found_inf), or None where this path does not apply."""
        lib = _lib.load()
        cap = int(lib.pnr_adam_max_tensors())
        todo = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("palettenerf_amd.optim.Adam: dense fp32 CUDA(HIP) parameters only (no CPU fallback)")
                if not (p.is_contiguous() and p.grad.is_contiguous()):
                    raise RuntimeError("palettenerf_amd.optim.Adam: parameters and gradients must be contiguous")
                todo.append((group, p))
        if not any(p.numel() for _, p in todo) or any(p.device != scale.device for _, p in todo):
            return None
        amp = self._amp_init(scale.device)
        params = [p for _, p in todo]
        if len(params) != len(amp["params"]) or any(a is not b for a, b in zip(params, amp["params"])):
            self._amp_reconcile()         # the skips of the pending steps belong to the parameters those steps had
            amp["params"] = params
        self._amp_poll(self.AMP_ROWS - 1)
        batches = {}
        for group, p in todo:
            beta1, beta2 = group["betas"]
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1               # optimistic: taken back when the host learns that the step was skipped
            key = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), int(st["step"].item()))
            batches.setdefault(key, []).append((p, st))
        items = [(p, self.state[p]) for p in params]
        found_inf, state = amp["found_inf"], amp["state"]
        ctl = _lib.AdamAmpCtl()
        ctl.scale, ctl.found_inf, ctl.state = scale.data_ptr(), found_inf.data_ptr(), state.data_ptr()
        ctl.skipped_base, ctl.parity = amp["skipped_base"], amp["calls"] & 1
        with torch.cuda.device(scale.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            found_inf.zero_()
            for i in range(0, len(items), cap):             # every check before every step: a late tensor's inf holds the early ones too
                arr = self._tensor_array(items[i:i + cap])
                _lib.check(lib.pnr_grad_check(arr, ctypes.c_uint32(len(arr)), ctypes.c_void_p(found_inf.data_ptr()), stream), "pnr_grad_check")
            for (lr, beta1, beta2, eps, step), members in batches.items():
                rows, n_rows = self._amp_rows(lr, beta1, beta2, eps, step)
                for i in range(0, len(members), cap):
                    arr = self._tensor_array(members[i:i + cap])
                    _lib.check(lib.pnr_adam_step_amp(arr, ctypes.c_uint32(len(arr)), rows, ctypes.c_uint32(n_rows), ctypes.byref(ctl), stream), "pnr_adam_step_amp")
            slot = amp["calls"] % amp["pinned"].shape[0]
            amp["pinned"][slot].copy_(state, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        amp["pending"].append((event, slot, (amp["calls"] & 1) ^ 1))
        amp["calls"] += 1
        for p in params:
            torch.autograd.graph.increment_version(p)
        return found_inf


class GradScaler(torch.amp.GradScaler):
    """torch.amp.GradScaler whose `step` does not return to the host when the optimiser is `Adam` (above): torch's `step` runs `unscale_` -- a
    read-and-write pass over every gradient -- and then reads found_inf back to decide whether to call optimizer.step(); here the finite check
    (pnr_grad_check) writes nothing but the flag and the step (pnr_adam_step_amp) unscales in its own pass and skips itself on the device.  Bit
    for bit torch's parameters, moments, `_scale`, `_growth_tracker` and step counts, skipped steps included.  Any other optimiser, an explicit
    `unscale_` before `step` (gradient clipping) and a disabled scaler take torch's path unchanged; so do `scale`, `update` and `state_dict`."""

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled or not isinstance(optimizer, Adam) or args or kwargs:
            return super().step(optimizer, *args, **kwargs)
        self._check_scale_growth_tracker("step")
        optimizer_state = self._per_optimizer_states[id(optimizer)]
        if optimizer_state["stage"] is not OptState.READY:
            return super().step(optimizer)
        found_inf = optimizer._amp_step(self._scale)
        if found_inf is None:
            return super().step(optimizer)
        optimizer_state["found_inf_per_device"] = {found_inf.device: found_inf}      # what the inherited update() consumes
        optimizer_state["stage"] = OptState.STEPPED
        return None


class ExponentialMovingAverage:
    """torch_ema 0.3's ExponentialMovingAverage (what the reference's Trainer builds over model.parameters(): nerf/utils.py, palette/utils.py,
    ema_decay 0.95) with the same constructor, attributes, methods and state_dict keys -- a reference checkpoint's 'ema' entry loads into it --
    whose `update` is one HIP launch per 32 tensors (pnr_ema_update: read p and s, write s; torch_ema's bits) instead of three elementwise
    launches per tensor, and no CPU path: parameters must be dense, contiguous, fp32 and on the device.

    `swap()` is new: it exchanges parameters and shadows in place (pnr_ema_swap) -- `store(); copy_to()` before an evaluation and, called again,
    `restore()` after it, without the third copy of every table -- and bumps the parameters' version counters, so every cache keyed on them (packed
    weights, interleaved tables, the occupancy mip) rebuilds by itself.  `average_parameters()` is swap / yield / swap.  `store`, `copy_to` and
    `restore` keep torch_ema's meaning and bump the versions of the parameters they write too (torch_ema writes through `.data`, which the caches
    only notice through the frame's source checksums)."""

    def __init__(self, parameters, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        parameters = list(parameters)
        self.shadow_params = [p.clone().detach() for p in parameters]      # every parameter passed, frozen ones included (torch_ema 0.3)
        self.collected_params = None
        self._params_refs = [weakref.ref(p) for p in parameters]
        self._swapped = False

    def _get_parameters(self, parameters):
        if parameters is None:
            parameters = [p() for p in self._params_refs]
            if any(p is None for p in parameters):
                raise ValueError("(One of) the parameters with which this ExponentialMovingAverage was initialized no longer exists (was garbage collected);"
                                 " please either provide `parameters` explicitly or keep the model to which they belong from being garbage collected.")
            return parameters
        parameters = list(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"Number of parameters passed as argument is different from number of shadow parameters maintained by this "
                             f"ExponentialMovingAverage ({len(parameters)} != {len(self.shadow_params)})")
        return parameters

    @staticmethod
    def decay_at(decay, num_updates):
        """torch_ema's warm-up, in Python doubles: the decay of update number `num_updates` (counted from 1)."""
        return min(decay, (1 + num_updates) / (10 + num_updates))

    def _device_pairs(self, parameters, what):
        """(parameter, shadow) pairs by device.  Every check before any launch: a rejected tensor must not leave earlier ones updated."""
        pairs = list(zip(parameters, self.shadow_params))
        for p, s in pairs:
            for t in (p, s):
                if t.is_sparse or t.dtype != torch.float32 or not t.is_cuda:
                    raise RuntimeError(f"palettenerf_amd.optim.ExponentialMovingAverage.{what}: dense fp32 CUDA(HIP) parameters and shadows only (no CPU fallback)")
                if not t.is_contiguous():
                    raise RuntimeError(f"palettenerf_amd.optim.ExponentialMovingAverage.{what}: parameters and shadows must be contiguous")
            if p.shape != s.shape or p.device != s.device:
                raise RuntimeError(f"palettenerf_amd.optim.ExponentialMovingAverage.{what}: a shadow does not match its parameter (shape or device)")
        by_device = {}
        for p, s in pairs:
            by_device.setdefault(p.device, []).append((p, s))
        return by_device

    def _launch(self, entry, by_device, *scalars):
        lib = _lib.load()
        cap = int(lib.pnr_adam_max_tensors())
        for device, pairs in by_device.items():
            with torch.cuda.device(device):      # the launch goes to the tensors' device, on torch's current stream there
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                for i in range(0, len(pairs), cap):
                    arr = (_lib.EmaTensor * len(pairs[i:i + cap]))()
                    for k, (p, s) in enumerate(pairs[i:i + cap]):
                        arr[k].param, arr[k].shadow, arr[k].n = p.data_ptr(), s.data_ptr(), p.numel()
                    _lib.check(getattr(lib, entry)(arr, ctypes.c_uint32(len(arr)), *scalars, stream), entry)

    @torch.no_grad()
    def update(self, parameters=None):
        parameters = self._get_parameters(parameters)
        if self._swapped:
            raise RuntimeError("palettenerf_amd.optim.ExponentialMovingAverage.update inside a swap: the parameters hold the averages (call swap() back first)")
        by_device = self._device_pairs(parameters, "update")
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = self.decay_at(decay, self.num_updates)
        self._launch("pnr_ema_update", by_device, ctypes.c_float(1.0 - decay))

    @torch.no_grad()
    def swap(self, parameters=None):
        """Exchange parameters and averages in place, one launch per 32 tensors and no copy; a second call puts both back, bit for bit."""
        parameters = self._get_parameters(parameters)
        self._launch("pnr_ema_swap", self._device_pairs(parameters, "swap"))
        self._swapped = not self._swapped
        for p in parameters:
            torch.autograd.graph.increment_version(p)   # written by a raw kernel: caches keyed on the version must see it

    @staticmethod
    def _copy(dst, src):
        if dst:
            with torch.no_grad():
                torch._foreach_copy_(dst, src)           # in place on the parameters themselves (not `.data`): their versions move

    def copy_to(self, parameters=None):
        self._copy(self._get_parameters(parameters), self.shadow_params)

    def store(self, parameters=None):
        self.collected_params = [p.detach().clone() for p in self._get_parameters(parameters)]

    def restore(self, parameters=None):
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        self._copy(self._get_parameters(parameters), self.collected_params)

    @contextlib.contextmanager
    def average_parameters(self, parameters=None):
        parameters = self._get_parameters(parameters)
        self.swap(parameters)
        try:
            yield
        finally:
            self.swap(parameters)

    def to(self, device=None, dtype=None):
        move = lambda t: t.to(device=device, dtype=dtype) if t.is_floating_point() else t.to(device=device)
        self.shadow_params = [move(s) for s in self.shadow_params]
        if self.collected_params is not None:
            self.collected_params = [move(c) for c in self.collected_params]

    def state_dict(self):
        """torch_ema's keys.  Inside a swap the shadows hold the raw parameters: refused."""
        if self._swapped:
            raise RuntimeError("palettenerf_amd.optim.ExponentialMovingAverage.state_dict inside a swap: the shadows hold the parameters (call swap() back first)")
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params, "collected_params": self.collected_params}

    def load_state_dict(self, state_dict):
        if self._swapped:
            raise RuntimeError("palettenerf_amd.optim.ExponentialMovingAverage.load_state_dict inside a swap (call swap() back first)")
        state_dict = copy.deepcopy(state_dict)
        decay, num_updates = state_dict["decay"], state_dict["num_updates"]
        shadow, collected = state_dict["shadow_params"], state_dict["collected_params"]
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        if not (num_updates is None or isinstance(num_updates, int)):
            raise ValueError("Invalid num_updates")
        if not (isinstance(shadow, list) and all(isinstance(s, torch.Tensor) for s in shadow)):
            raise ValueError("shadow_params must be a list of Tensors")
        if collected is not None:
            if not (isinstance(collected, list) and all(isinstance(c, torch.Tensor) for c in collected)):
                raise ValueError("collected_params must be a list of Tensors")
            if len(collected) != len(shadow):
                raise ValueError("collected_params and shadow_params had different lengths")
        if len(shadow) != len(self._params_refs):
            raise ValueError("Tried to `load_state_dict()` with the wrong number of parameters in the saved state.")
        params = [p() for p in self._params_refs]
        if not any(p is None for p in params):             # as torch.optim.Optimizer does: onto the parameters' device and dtype
            cast = lambda t, p: t.to(device=p.device, dtype=p.dtype) if p.is_floating_point() else t.to(device=p.device)
            shadow = [cast(s, p) for s, p in zip(shadow, params)]
            if collected is not None:
                collected = [cast(c, p) for c, p in zip(collected, params)]
        self.decay, self.num_updates, self.shadow_params, self.collected_params = decay, num_updates, shadow, collected
