"""The loss-scaled optimiser step on the device: optim.GradScaler + optim.Adam (pnr_grad_check, pnr_adam_step_amp) against the control
torch.amp.GradScaler + torch.optim.Adam (default foreach) on cloned tensors -- torch.equal on parameters, exp_avg, exp_avg_sq, _scale and
_growth_tracker, and the state_dict's step counts, after every step, skipped steps included.

Shapes: 1, 2047, 2049 and 3 * 2048 + 5 elements and an empty tensor (one chunk, the chunk edge, a ragged tail) in two param groups; 40 tensors of
3 elements for the 32-tensor cap.  The no-synchronisation test uses torch.cuda.set_sync_debug_mode("error")."""
import copy

import numpy as np
import pytest
import torch

from palettenerf_amd import optim

pytestmark = pytest.mark.gpu
SIZES = (1, 2047, 2049, 3 * 2048 + 5, 0)
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
SCALER = dict(init_scale=2.0 ** 15, growth_interval=2)
INF, NAN = float("inf"), float("nan")
# step -> (tensor, element, value): consecutive skips in the first element of the first tensor, the last element of the last (non-empty) tensor,
# the second chunk of the large one
SEQUENCE = {3: (0, 0, INF), 4: (0, 0, INF), 8: (3, 3 * 2048 + 4, -INF), 11: (3, 2048 + 77, NAN)}


class Leg:
    """One optimiser + scaler over its own copy of the tensors."""

    def __init__(self, cuda, sizes, adam, scaler, seed=0, **scaler_kw):
        g = torch.Generator().manual_seed(seed)
        self.params = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in sizes]
        half = max(1, len(sizes) // 2)
        self.groups = lambda ps: [dict(params=ps[:half]), dict(params=ps[half:], lr=3e-3)]
        self.opt = adam(self.groups(self.params), **HYPER)
        self.scaler = scaler("cuda", **{**SCALER, **scaler_kw})
        self.one = torch.ones((), device=cuda)

    def set_grads(self, base, plant=None):
        """Gradients = fixed random fp32 x the current scale (formed on the device: no read of the scale), with one value planted."""
        scale = self.scaler.scale(self.one) if self.scaler.is_enabled() else self.one       # (also what initialises _scale)
        for k, (p, b) in enumerate(zip(self.params, base)):
            p.grad = b * scale
            if plant is not None and plant[0] == k:
                p.grad[plant[1]] = plant[2]

    def step(self, base, plant=None):
        self.set_grads(base, plant)
        self.scaler.step(self.opt)
        self.scaler.update()


def base_grads(cuda, sizes, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g).to(cuda) for n in sizes] for _ in range(steps)]


def assert_same(ours, ctrl, where):
    assert torch.equal(ours.scaler._scale, ctrl.scaler._scale) and torch.equal(ours.scaler._growth_tracker, ctrl.scaler._growth_tracker), where
    sd_o, sd_c = ours.opt.state_dict()["state"], ctrl.opt.state_dict()["state"]
    for i, (p, q) in enumerate(zip(ours.params, ctrl.params)):
        assert torch.equal(p, q), (where, "param", i)
        st = ctrl.opt.state.get(q)
        if st:      # (torch makes a tensor's state at its first step that is not skipped; until then ours is zeros at step 0)
            want = st["exp_avg"], st["exp_avg_sq"], float(sd_c[i]["step"])
        else:
            want = torch.zeros_like(q), torch.zeros_like(q), 0.0
        assert torch.equal(ours.opt.state[p]["exp_avg"], want[0]) and torch.equal(ours.opt.state[p]["exp_avg_sq"], want[1]), (where, "moments", i)
        assert float(sd_o[i]["step"]) == want[2], (where, "step", i, float(sd_o[i]["step"]), want[2])


def run_sequence(cuda, steps=14):
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, optim.GradScaler), Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, SIZES, steps + 3)
    scales = []
    for i in range(steps):
        before = [p.detach().clone() for p in ours.params]
        ours.step(base[i], SEQUENCE.get(i))
        ctrl.step(base[i], SEQUENCE.get(i))
        assert_same(ours, ctrl, f"step {i}")
        moved = not torch.equal(before[3], ours.params[3].detach())
        assert moved == (i not in SEQUENCE), f"step {i}"              # the finite steps really update, the others leave every bit
        scales.append(float(ours.scaler._scale))
    assert max(scales) > SCALER["init_scale"] > min(scales)          # the scale grew, backed off and grew again
    assert int(ours.opt._amp["state"][2]) == 0
    return ours, ctrl, base


def test_fourteen_steps_with_skips_are_torchs_bits(cuda):
    run_sequence(cuda)


def test_checkpoint_into_torch_adam_continues_bit_equal(cuda):
    ours, ctrl, base = run_sequence(cuda)
    sd = ours.opt.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [float(s["step"]) for s in ctrl.opt.state_dict()["state"].values()] == [10.0] * len(SIZES)
    fresh = Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    with torch.no_grad():
        for p, q in zip(fresh.params, ours.params):
            p.copy_(q)
    fresh.opt.load_state_dict(copy.deepcopy(sd))                      # (load_state_dict keeps the tensors it is given)
    fresh.scaler = ctrl.scaler                                        # the control's scaler goes on with the fresh optimiser
    for i in range(14, 17):
        ours.step(base[i])
        fresh.step(base[i])
        assert_same(ours, fresh, f"step {i} after the checkpoint")


def test_more_tensors_than_one_launch_takes_every_check_runs_before_every_step(cuda):
    sizes = (3,) * 40
    ours, ctrl = Leg(cuda, sizes, optim.Adam, optim.GradScaler), Leg(cuda, sizes, torch.optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, sizes, 3)
    ours.step(base[0]), ctrl.step(base[0])
    assert_same(ours, ctrl, "finite step")
    first = ours.params[0].detach().clone()
    ours.step(base[1], (35, 1, INF)), ctrl.step(base[1], (35, 1, INF))
    assert torch.equal(ours.params[0].detach(), first)               # tensor 0 is in the first launch, the inf in the second
    assert_same(ours, ctrl, "inf in tensor 35")
    ours.step(base[2]), ctrl.step(base[2])
    assert_same(ours, ctrl, "finite step after the skip")
    assert not torch.equal(ours.params[0].detach(), first) and int(ours.opt._amp["state"][2]) == 0


def test_more_consecutive_skips_than_rows(cuda):
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, optim.GradScaler), Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, SIZES, 24)
    for i in range(2):
        ours.step(base[i]), ctrl.step(base[i])
    for i in range(2, 2 + 19):                                        # 2 * 8 + 3, and nothing here reads anything back
        ours.step(base[i], (1, 5, NAN))
    for i in range(2, 2 + 19):
        ctrl.step(base[i], (1, 5, NAN))
    for i in range(21, 24):
        ours.step(base[i]), ctrl.step(base[i])
    assert_same(ours, ctrl, "after 19 skipped and 3 finite steps")
    assert float(ours.opt.state_dict()["state"][0]["step"]) == 5.0 and int(ours.opt._amp["state"][2]) == 0


def test_an_explicit_unscale_takes_torchs_path(cuda):
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, optim.GradScaler), Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, SIZES, 3)
    for i, plant in enumerate((None, (2, 7, INF), None)):
        for leg in (ours, ctrl):
            leg.set_grads(base[i], plant)
            leg.scaler.unscale_(leg.opt)
            leg.scaler.step(leg.opt)
            leg.scaler.update()
        assert "_amp" not in ours.opt.__dict__                       # the device path never ran
        for p, q in zip(ours.params, ctrl.params):
            assert torch.equal(p, q) and (p.grad is None or torch.equal(p.grad, q.grad))
        assert torch.equal(ours.scaler._scale, ctrl.scaler._scale)
    assert [float(s["step"]) for s in ours.opt.state_dict()["state"].values()] == [2.0] * len(SIZES)


def test_a_disabled_scaler_is_the_plain_step(cuda):
    ours, plain = Leg(cuda, SIZES, optim.Adam, optim.GradScaler, enabled=False), Leg(cuda, SIZES, optim.Adam, optim.GradScaler, enabled=False)
    base = base_grads(cuda, SIZES, 2)
    for i in range(2):
        ours.step(base[i])
        plain.set_grads(base[i])
        plain.opt.step()
        for p, q in zip(ours.params, plain.params):
            assert torch.equal(p, q)
    assert "_amp" not in ours.opt.__dict__


def test_the_float_grad_scale_of_the_plain_step_is_unchanged(cuda):
    """optim.Adam.step with grad_scale = a float: torch's unscale_ + step on the same scaled gradients."""
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, optim.GradScaler), Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, SIZES, 2)
    for i in range(2):
        ctrl.set_grads(base[i])
        for p, q in zip(ours.params, ctrl.params):
            p.grad = q.grad.clone()
        ours.opt.grad_scale = SCALER["init_scale"]
        ours.opt.step()
        ctrl.scaler.unscale_(ctrl.opt)
        ctrl.scaler.step(ctrl.opt)
        ctrl.scaler._per_optimizer_states.clear()                     # (no update(): the scale stays 2^15 for both steps)
        for p, q in zip(ours.params, ctrl.params):
            assert torch.equal(p, q)
            assert torch.equal(ours.opt.state[p]["exp_avg_sq"], ctrl.opt.state[q]["exp_avg_sq"])
    assert ours.opt.grad_scale == SCALER["init_scale"]


def test_torchs_scaler_with_this_adam_still_works_as_before(cuda):
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, torch.amp.GradScaler), Leg(cuda, SIZES, torch.optim.Adam, torch.amp.GradScaler)
    assert not getattr(ours.opt, "_step_supports_amp_scaling", False) and ours.opt.grad_scale is None
    base = base_grads(cuda, SIZES, 3)
    for i, plant in enumerate((None, (0, 0, INF), None)):
        ours.step(base[i], plant), ctrl.step(base[i], plant)
        for p, q in zip(ours.params, ctrl.params):
            assert torch.equal(p, q)


def test_step_and_update_do_not_synchronise(cuda):
    """Method: torch.cuda.set_sync_debug_mode("error"), under which any synchronising torch call raises."""
    ours, ctrl = Leg(cuda, SIZES, optim.Adam, optim.GradScaler), Leg(cuda, SIZES, optim.Adam, torch.amp.GradScaler)
    base = base_grads(cuda, SIZES, 6)
    ours.step(base[0]), ctrl.step(base[0])                            # (allocations and the library's first load, outside the mode)
    for leg in (ours, ctrl):
        for i in range(1, 6):
            leg.set_grads(base[i], (0, 0, INF) if i == 2 else None)
            leg.grads = getattr(leg, "grads", []) + [[p.grad for p in leg.params]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for grads in ours.grads[:4]:
            for p, g in zip(ours.params, grads):
                p.grad = g
            ours.scaler.step(ours.opt)
            ours.scaler.update()
        for p, g in zip(ctrl.params, ctrl.grads[0]):
            p.grad = g
        with pytest.raises(RuntimeError, match="synchroniz"):
            ctrl.scaler.step(ctrl.opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(ours.opt.state_dict()["state"][0]["step"]) == 4.0    # five steps, one skipped


def test_step_and_update_are_at_most_five_launches(cuda):
    from torch.profiler import ProfilerActivity, profile
    ours = Leg(cuda, SIZES, optim.Adam, optim.GradScaler)
    base = base_grads(cuda, SIZES, 3)
    ours.step(base[0])
    ours.step(base[1])
    ours.set_grads(base[2])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ours.scaler.step(ours.opt)
        ours.scaler.update()
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    print("kernels of one step + update:", kernels)
    assert any("k_grad_check" in k for k in kernels) and any("k_adam" in k for k in kernels)
    assert len(kernels) <= 5, kernels


# ---------------------------------------------------------------- end to end: trainset.train_epoch(fp16=True)

V, H, W = 3, 37, 53
RENDER = dict(dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4)
LAMBDAS = dict(lambda_sparsity=2e-4, lambda_offsets=0.03, lambda_view_dep=0.1, lambda_weight=0.05, lambda_palette=1e-3)


def small_model(cuda):
    from palettenerf_amd import network, raymarching, renderer, scene
    g = np.random.default_rng(408)
    hist = g.random((4, 8, 8, 8)).astype(np.float32)
    hist = (hist / hist.sum(0, keepdims=True)).astype(np.float32)
    torch.manual_seed(0)
    m = network.PaletteNetwork(renderer.default_opt(test=False), bound=2, cuda_ray=True, min_near=0.02)
    scene.seed_field_(m, 0)
    m.initialize_palette([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.8, 0.8, 0.7]], hist_weights=np.moveaxis(hist, 0, -1))
    m = m.to(cuda).train()
    with torch.no_grad():
        m.basis_color += 0.05
    m.density_grid.copy_(torch.from_numpy(scene.slab_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    return m


def small_set(N):
    from palettenerf_amd import scene, trainset
    g = np.random.default_rng(H * 1000 + W + 4)
    images = g.random((V, H, W, 4), dtype=np.float32)
    poses = []
    for i in range(V):
        a = 2 * np.pi * i / V
        p = np.eye(4, dtype=np.float32)
        p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = [1, 0, 0], [0, -1, 0], [0, 0, -1], [0.3 * np.cos(a), 0.3 * np.sin(a), 1.5]
        poses.append(p)
    return trainset.TrainSet(images, np.stack(poses), scene.intrinsics_from_fov(H, W, 0.9), H, W, N, storage="fp16")


@pytest.mark.parametrize("init_scale", [2.0 ** 10, 2.0 ** 40])
def test_two_fp16_train_epoch_steps_equal_torchs_scaler(cuda, init_scale):
    """Both scalers drive optim.Adam; from 2^40 the first step overflows fp16 and is skipped."""
    from palettenerf_amd import trainset
    result = []
    for scaler_cls in (optim.GradScaler, torch.amp.GradScaler):
        m = small_model(cuda)
        ts = small_set(257)
        opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        scaler = scaler_cls("cuda", init_scale=init_scale)
        before = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
        torch.manual_seed(9)
        avg, step = trainset.train_epoch(m, ts, opt, scaler=scaler, fp16=True, global_step=15, max_steps=2, render_kwargs=RENDER,
                                         generator=torch.Generator().manual_seed(1), **LAMBDAS)
        assert step == 17
        steps = {float(s["step"]) for s in opt.state_dict()["state"].values()} or {0.0}    # (torch's path makes no state before a step is taken)
        result.append(({n: p.detach().clone() for n, p in m.named_parameters()}, before, steps, scaler.get_scale()))
    (ours, before, steps, scale), (theirs, _, steps_t, scale_t) = result
    print(f"init_scale {init_scale:g}: step counts {steps} / {steps_t}, scale after two steps {scale:g} / {scale_t:g}")
    assert steps == steps_t and scale == scale_t
    assert (max(steps) <= 1.0) if init_scale > 2.0 ** 30 else (steps == {2.0})
    for n in ours:
        assert torch.equal(ours[n], theirs[n]), n
    assert any(not torch.equal(ours[n], before[n]) for n in before) == (max(steps) > 0)
