"""The weights' average on the device: optim.ExponentialMovingAverage (pnr_ema_update, pnr_ema_swap) against the control of
tests/ema_reference.py, torch_ema's three torch expressions per tensor on the same device, bit for bit: shadows, num_updates and, where an
optimiser runs, parameters, moments and step counts against torch.optim.Adam / torch.amp.GradScaler.

Shapes are test_gpu_amp.py's -- 1, 2047, 2049 and 3 * 2048 + 5 elements and an empty tensor (one chunk, the chunk edge, a ragged tail) -- plus a
255-element tensor; 34 tensors where the 32-tensor cap of one launch matters."""
import warnings

import pytest
import torch

from palettenerf_amd import optim
from tests import ema_reference as ref
from tests import test_gpu_amp as amp

pytestmark = pytest.mark.gpu
SIZES = amp.SIZES + (255,)
SIZES34 = SIZES + (3,) * 28
DECAY = 0.95
INF = float("inf")


def bits(a, b):
    """Equal bit for bit (torch.equal would take -0.0 for 0.0)."""
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def all_bits(xs, ys):
    return len(xs) == len(ys) and all(bits(x, y) for x, y in zip(xs, ys))


def snapshot(xs):
    return [x.detach().clone() for x in xs]


# ---------------------------------------------------------------- stand-alone: pnr_ema_update

def test_180_updates_are_the_controls_bits(cuda):
    """Past the warm-up's switch at update 170; 34 tensors = two launches; tensor 2 is never perturbed: a parameter equal to its shadow keeps
    every bit of it."""
    assert len(SIZES34) == 34
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in SIZES34]
    params[1].requires_grad_(False)                                   # frozen ones are averaged too
    noise = [torch.randn(n, generator=g).to(cuda) * 1e-2 for n in SIZES34]
    moving = [p for i, p in enumerate(params) if i != 2]
    moving_noise = [x for i, x in enumerate(noise) if i != 2]
    ours, ctrl = optim.ExponentialMovingAverage(params, DECAY), ref.ControlEMA(params, DECAY)
    still = params[2].detach().clone()
    for k in range(180):
        with torch.no_grad():
            torch._foreach_add_(moving, moving_noise, alpha=(1 + k % 5) * (-1.0) ** (k // 3))
        ours.update()
        ctrl.update()
        if k % 45 == 44 or k in (0, 168, 169, 170):
            assert all_bits(ours.shadow_params, ctrl.shadow_params), f"update {k + 1}"
    assert ours.num_updates == ctrl.num_updates == 180
    assert all_bits(ours.shadow_params, ctrl.shadow_params)
    assert bits(ours.shadow_params[2], still) and bits(params[2], still)
    assert not bits(ours.shadow_params[3], params[3]) and ours.shadow_params[4].numel() == 0
    # use_num_updates=False: the constant decay from the first update on
    ours, ctrl = optim.ExponentialMovingAverage(params[:6], 0.5, use_num_updates=False), ref.ControlEMA(params[:6], 0.5, use_num_updates=False)
    ours.update(), ctrl.update()
    assert ours.num_updates is None and all_bits(ours.shadow_params, ctrl.shadow_params)


# ---------------------------------------------------------------- after optim.Adam's plain step

class PlainLeg:
    """Six optimised tensors in two param groups with different lr, one tensor in the optimiser that never gets a gradient, one tracked tensor
    outside the optimiser (moved by hand)."""

    def __init__(self, cuda, adam, ema):
        g = torch.Generator().manual_seed(0)
        self.ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in SIZES]
        self.no_grad = torch.nn.Parameter(torch.randn(300, generator=g).to(cuda))
        self.outside = torch.nn.Parameter(torch.randn(2050, generator=g).to(cuda))
        self.opt = adam([dict(params=self.ps[:3]), dict(params=self.ps[3:] + [self.no_grad], lr=3e-3)], **amp.HYPER)
        self.tracked = self.ps + [self.no_grad, self.outside]
        self.ema = ema(self.tracked, DECAY)

    def step(self, base, drift):
        for p, b in zip(self.ps, base):
            p.grad = b.clone()
        with torch.no_grad():
            self.outside.add_(drift)
        self.opt.step()
        self.ema.update()

    def state(self):
        sd = self.opt.state_dict()["state"]
        return dict(params=snapshot(self.tracked), shadows=snapshot(self.ema.shadow_params),
                    exp_avg=snapshot([self.opt.state[p]["exp_avg"] for p in self.ps]), exp_avg_sq=snapshot([self.opt.state[p]["exp_avg_sq"] for p in self.ps]),
                    steps=[float(sd[i]["step"]) for i in sorted(sd)], num_updates=self.ema.num_updates)


def test_fourteen_plain_steps_with_an_update_each_are_torchs_and_the_controls_bits(cuda):
    legs = dict(ours=PlainLeg(cuda, optim.Adam, optim.ExponentialMovingAverage), control=PlainLeg(cuda, torch.optim.Adam, ref.ControlEMA))
    base = amp.base_grads(cuda, SIZES, 14)
    g = torch.Generator().manual_seed(5)
    drifts = [torch.randn(2050, generator=g).to(cuda) * 1e-2 for _ in range(14)]
    for i in range(14):
        states = {}
        for name, leg in legs.items():
            leg.step(base[i], drifts[i])
            states[name] = leg.state()
        want = states["control"]
        for name in ("ours",):
            got = states[name]
            for key in ("params", "shadows", "exp_avg", "exp_avg_sq"):
                assert all_bits(got[key], want[key]), (i, name, key, [k for k, (x, y) in enumerate(zip(got[key], want[key])) if not bits(x, y)])
            assert got["steps"] == want["steps"] == [float(i + 1)] * len(SIZES) and got["num_updates"] == want["num_updates"] == i + 1, (i, name)
    leg = legs["ours"]
    assert not any(bits(s, p) for s, p in zip(leg.ema.shadow_params[:4], leg.tracked[:4]))
    assert bits(leg.ema.shadow_params[6], leg.no_grad)                # never moved: the average of a constant is the constant, bit for bit


# ---------------------------------------------------------------- after the loss-scaled step

def test_fourteen_loss_scaled_steps_with_skips_are_torchs_and_the_controls_bits(cuda):
    """test_gpu_amp.py's SEQUENCE of planted inf / nan, plus one in the last element of the last of the 34 tensors (the second launch).  On a
    skipped step the parameters keep every bit and the shadows still move (the reference's update() does not ask whether the scaler skipped).
    update() after optim.GradScaler's device path reads nothing back: the step's skip is not known on the host when it is enqueued."""
    sequence = {**amp.SEQUENCE, 12: (33, 2, -INF)}
    legs = dict(ours=amp.Leg(cuda, SIZES34, optim.Adam, optim.GradScaler), control=amp.Leg(cuda, SIZES34, torch.optim.Adam, torch.amp.GradScaler))
    emas = {name: (ref.ControlEMA if name == "control" else optim.ExponentialMovingAverage)(leg.params, DECAY) for name, leg in legs.items()}
    base = amp.base_grads(cuda, SIZES34, 14)
    for i in range(14):
        before = snapshot(legs["ours"].params), snapshot(emas["ours"].shadow_params)
        for name, leg in legs.items():
            leg.step(base[i], sequence.get(i))
            emas[name].update()
        for name in ("ours",):
            amp.assert_same(legs[name], legs["control"], f"step {i} ({name})")
            assert all_bits(legs[name].params, legs["control"].params), (i, name)
            assert all_bits(emas[name].shadow_params, emas["control"].shadow_params), (i, name)
            assert emas[name].num_updates == emas["control"].num_updates == i + 1
        if i in sequence:
            assert all_bits(legs["ours"].params, before[0]), f"step {i}: a skipped step keeps every bit of the parameters"
            assert not bits(emas["ours"].shadow_params[3], before[1][3]) and not bits(emas["ours"].shadow_params[33], before[1][33]), f"step {i}: the shadows still move"
        else:
            assert not bits(legs["ours"].params[3], before[0][3]), f"step {i}"
    assert int(legs["ours"].opt._amp["state"][2]) == 0
    assert float(legs["ours"].opt.state_dict()["state"][0]["step"]) == 14.0 - len(sequence)


# ---------------------------------------------------------------- launches and synchronisation

def kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_an_update_is_one_launch_per_32_tensors_and_does_not_synchronise(cuda):
    """The launches are counted with torch's profiler, as test_gpu_amp.py does; synchronisation with torch.cuda.set_sync_debug_mode("error"), under
    which any synchronising torch call raises.  The control runs three launches per non-empty tensor."""
    g = torch.Generator().manual_seed(0)
    for sizes, launches in ((SIZES, 1), (SIZES34, 2)):
        params = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in sizes]
        ema, ctrl = optim.ExponentialMovingAverage(params, DECAY), ref.ControlEMA(params, DECAY)
        ema.update(), ctrl.update()                                   # (the library's first load, outside the mode)
        with torch.no_grad():
            torch._foreach_mul_(params, 1.01)

        def update():
            torch.cuda.set_sync_debug_mode("error")
            try:
                ema.update()
            finally:
                torch.cuda.set_sync_debug_mode("default")

        ours, theirs = kernels_of(update), kernels_of(ctrl.update)
        print(len(sizes), "tensors:", ours, len(theirs), "launches of the control")
        assert len(ours) == launches and all("k_ema" in k for k in ours), ours
        assert len(theirs) == 3 * sum(1 for n in sizes if n)
        assert all_bits(ema.shadow_params, ctrl.shadow_params)


# ---------------------------------------------------------------- swap and the caches keyed on the parameters' versions

def frame_model(cuda):
    from palettenerf_amd import network, raymarching, renderer, scene
    m = network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, density_scale=30.0, min_near=0.2)
    scene.seed_field_(m, 17)
    m = m.to(cuda).eval()
    m.density_grid.copy_(torch.from_numpy(scene.brick_density_grid()).to(cuda))
    raymarching.packbits(m.density_grid, 0.5, m.density_bitfield)
    m.march_mode, m.fused_field = "native", True
    return m


def test_swap_twice_restores_every_bit_and_the_native_frame_follows_without_invalidate(cuda):
    from palettenerf_amd import scene
    m = frame_model(cuda)
    pose = torch.from_numpy(scene.lookat_pose())[None]
    ro, rd = scene.get_rays(pose, scene.intrinsics_from_fov(48, 48), 48, 48)
    ro, rd = ro.to(cuda), rd.to(cuda)

    def frame(model):
        with torch.no_grad(), warnings.catch_warnings():
            # the frame's source checksums would notice a write the version counters missed, rebuild, render again and warn: not wanted here
            warnings.filterwarnings("error", message=".*rewritten behind torch's version counters.*")
            image = model.render(ro, rd, dt_gamma=0, perturb=False, max_steps=1024, T_thresh=1e-4, gui_mode=False)["image"]
        return torch.nan_to_num(image, nan=-7.0).clone()

    params = list(m.parameters())
    ema = optim.ExponentialMovingAverage(params, DECAY)
    with torch.no_grad():                                # averages that differ from the parameters, tensor by tensor
        for k, s in enumerate(ema.shadow_params):
            s.mul_(0.8 + 0.01 * (k % 7))
    p0, s0 = snapshot(params), snapshot(ema.shadow_params)
    original = frame(m)
    fresh = frame_model(cuda)
    with torch.no_grad():
        for p, s in zip(fresh.parameters(), s0):
            p.copy_(s)
    want = frame(fresh)
    assert float((want - original).abs().max()) > 1e-3

    versions = [p._version for p in params]
    ema.swap()
    assert all_bits(params, s0) and all_bits(ema.shadow_params, p0) and all(p._version > v for p, v in zip(params, versions))
    with pytest.raises(RuntimeError, match="inside a swap"):
        ema.state_dict()
    with pytest.raises(RuntimeError, match="inside a swap"):
        ema.update()
    ema.swap()
    assert all_bits(params, p0) and all_bits(ema.shadow_params, s0)
    assert ema.state_dict()["num_updates"] == 0

    with ema.average_parameters():
        inside = frame(m)
    after = frame(m)
    assert torch.equal(inside, want)
    assert torch.equal(after, original)
    assert all_bits(params, p0) and all_bits(ema.shadow_params, s0)
    # store / copy_to / restore: torch_ema's meaning, and the frame follows them as well
    ema.store()
    ema.copy_to()
    assert all_bits(params, s0) and all_bits(ema.shadow_params, s0) and all_bits(ema.collected_params, p0)
    assert torch.equal(frame(m), want)
    ema.restore()
    assert all_bits(params, p0) and torch.equal(frame(m), original)


# ---------------------------------------------------------------- trainset.train_epoch(..., ema=)

def test_train_epoch_updates_the_average_where_the_reference_does(cuda):
    """Two -O steps of train_epoch on test_gpu_amp.py's small set-up with ema=: the same pass without it and the control's update applied by hand
    where the reference's train_one_epoch calls it -- once, after the pass (palette/utils.py:746-747)."""
    from palettenerf_amd import trainset
    result = []
    for ours in (True, False):
        m = amp.small_model(cuda)
        ts = amp.small_set(257)
        opt = optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        params = list(m.parameters())
        ema = (optim.ExponentialMovingAverage if ours else ref.ControlEMA)(params, DECAY)
        torch.manual_seed(9)
        avg, step = trainset.train_epoch(m, ts, opt, scaler=optim.GradScaler("cuda", init_scale=2.0 ** 10), fp16=True, global_step=15, max_steps=2,
                                         render_kwargs=amp.RENDER, generator=torch.Generator().manual_seed(1), ema=ema if ours else None, **amp.LAMBDAS)
        assert step == 17
        if not ours:
            ema.update()
        result.append((snapshot(params), snapshot(ema.shadow_params), ema.num_updates, avg))
    (p_o, s_o, n_o, avg_o), (p_c, s_c, n_c, avg_c) = result
    assert n_o == n_c == 1 and avg_o == avg_c
    assert all_bits(p_o, p_c) and all_bits(s_o, s_c)
    moved = [k for k, (p, s) in enumerate(zip(p_o, s_o)) if not bits(p, s)]
    assert moved, "two steps moved no parameter away from its average"


# ---------------------------------------------------------------- misuse: raises before anything is touched

def test_what_the_kernels_do_not_take_raises_and_leaves_everything_untouched(cuda):
    """A strided, a half and a double parameter, each behind a good one in the list: nothing is launched, num_updates stays."""
    for odd in (torch.nn.Parameter(torch.randn(8, 6, device=cuda).t()), torch.nn.Parameter(torch.randn(9, device=cuda).half()),
                torch.nn.Parameter(torch.randn(9, device=cuda).double())):
        good = torch.nn.Parameter(torch.randn(5, device=cuda))
        e = optim.ExponentialMovingAverage([good, odd], DECAY)
        with torch.no_grad():
            good.add_(1.0)
        shadow, value, version = e.shadow_params[0].clone(), good.detach().clone(), good._version
        for call in (e.update, e.swap):
            with pytest.raises(RuntimeError, match="contiguous|fp32"):
                call()
        with pytest.raises(RuntimeError, match="contiguous|fp32"):
            with e.average_parameters():
                pass
        assert e.num_updates == 0 and bits(e.shadow_params[0], shadow) and bits(good, value) and good._version == version and not e._swapped
    with pytest.raises(ValueError, match="Number of parameters"):
        e.update([good])
