"""CPU suite: the one-shot flex deferral that dropin.fuse_field arms behind every fused PaletteNetwork.forward (raymarching.arm_flex_deferral_in_iteration)
defers only the composites of the march iteration that is open on this thread.  The kernel calls are replaced by recorders: what is checked is WHEN a
composite_rays_flex reaches the library (at once, or queued until the iteration's composite_rays), not what it computes."""
import pytest
import torch

from palettenerf_amd import raymarching


@pytest.fixture()
def recorded(monkeypatch):
    calls = []
    monkeypatch.setattr(raymarching, "_composite_rays_flex_now", lambda n_alive, n_step, n_channel, rays_alive, rays_t, sigmas, inp, deltas, weights_sum, output,
                        T_thresh: calls.append(("now", rays_alive, output)))
    monkeypatch.setattr(raymarching, "composite_rays_flex_multi", lambda n_alive, n_step, rays_alive, rays_t, sigmas, deltas, weights_sum, maps, T_thresh:
                        calls.append(("multi", rays_alive, [m[2] for m in maps])))
    monkeypatch.setattr(raymarching, "_march_rays_now", lambda *a: ("xyzs", "dirs", "deltas"))
    monkeypatch.setattr(raymarching, "_composite_rays_now", lambda *a: calls.append(("composite",)) or tuple())
    q = raymarching._flex_queues.q
    was = raymarching.defer_flex_composites(False)
    q.iteration, q.armed, q.bound = None, False, None
    yield calls
    q.flush()
    q.iteration, q.armed, q.bound = None, False, None
    raymarching.defer_flex_composites(was)


_SHARED = {}


def _flex(n_alive, alive, out):
    """One composite_rays_flex of an iteration: the arguments an iteration's calls share are the same tensors for every call with this n_alive."""
    n_step = 2
    M = n_alive * n_step
    if n_alive not in _SHARED:
        _SHARED[n_alive] = (torch.zeros(n_alive, 2), torch.zeros(M), torch.zeros(M, 2), torch.zeros(n_alive))
    rays_t, sigmas, deltas, weights_sum = _SHARED[n_alive]
    raymarching.composite_rays_flex(n_alive, n_step, 3, alive, rays_t, sigmas, torch.zeros(M, 3), deltas, weights_sum, out, 1e-4)


def _march(n_alive, alive):
    return raymarching.march_rays(n_alive, 2, alive, torch.zeros(n_alive, 2), torch.zeros(n_alive, 3), torch.zeros(n_alive, 3), 2.0, None, 1, 128, None, None)


def test_flex_deferral_is_armed_only_inside_a_march_iteration_and_only_for_its_rays(recorded):
    calls = recorded
    alive_a = torch.arange(8, dtype=torch.int32)
    alive_b = torch.arange(8, dtype=torch.int32)
    o1, o2, o3, o4, o5 = (torch.zeros(8, 3) for _ in range(5))
    # a fused forward outside any loop (a point query, an export script): nothing is open, nothing is armed, the flex call runs at once
    raymarching.arm_flex_deferral_in_iteration()
    assert not raymarching._flex_queues.q.armed
    _flex(8, alive_a, o1)
    assert calls == [("now", alive_a, o1)]
    # an iteration of the reference's loop: march -> fused forward (arms) -> flex calls on the iteration's rays are queued ...
    calls.clear()
    _march(8, alive_a)
    raymarching.arm_flex_deferral_in_iteration()
    _flex(8, alive_a, o2)
    _flex(8, alive_a, o3)
    assert calls == []
    # ... until a flex call on other rays: the queue goes out first (one launch for the two), then that call, at once; the deferral has ended
    _flex(8, alive_b, o4)
    assert [c[0] for c in calls] == ["multi", "now"]
    assert calls[0][1] is alive_a and calls[0][2][0] is o2 and calls[0][2][1] is o3
    assert calls[1][1] is alive_b and calls[1][2] is o4
    calls.clear()
    _flex(8, alive_a, o5)
    assert calls == [("now", alive_a, o5)]
    # the same rays with another n_alive are not the iteration either
    calls.clear()
    _march(8, alive_a)
    raymarching.arm_flex_deferral_in_iteration()
    _flex(4, alive_a, o1)
    assert calls == [("now", alive_a, o1)]
    # the loop's own order: march, arm, flex x 2, composite_rays -> the two flex composites reach the library as one launch in front of the composite
    calls.clear()
    _march(8, alive_a)
    raymarching.arm_flex_deferral_in_iteration()
    _flex(8, alive_a, o2)
    _flex(8, alive_a, o3)
    raymarching.composite_rays(8, 2, alive_a, None, None, None, None, None, None, None, 1e-4)
    assert [c[0] for c in calls] == ["multi", "composite"]
    # the composite closed the iteration: a later forward arms nothing
    calls.clear()
    raymarching.arm_flex_deferral_in_iteration()
    _flex(8, alive_a, o4)
    assert calls == [("now", alive_a, o4)]


def test_persistent_flex_deferral_keeps_queueing_any_rays(recorded):
    """defer_flex_composites(True) is the explicit, persistent switch: every flex call is queued (no open iteration needed) until the next writer of
    what they read; calls with other shared arguments flush what is queued first."""
    calls = recorded
    alive_a = torch.arange(8, dtype=torch.int32)
    alive_b = torch.arange(8, dtype=torch.int32)
    o1, o2 = torch.zeros(8, 3), torch.zeros(8, 3)
    raymarching.defer_flex_composites(True)
    _flex(8, alive_a, o1)
    assert calls == []
    _flex(8, alive_b, o2)
    assert calls == [("now", alive_a, o1)]
    raymarching.flush_flex_composites()
    assert calls[-1] == ("now", alive_b, o2)
    raymarching.defer_flex_composites(False)
    # and the caller's own one-shot arming (a loop driven by hand) defers whatever follows up to the composite, march iteration or not
    calls.clear()
    raymarching.arm_flex_deferral()
    _flex(8, alive_a, o1)
    _flex(8, alive_a, o2)
    assert calls == []
    raymarching.composite_rays(8, 2, alive_a, None, None, None, None, None, None, None, 1e-4)
    assert [c[0] for c in calls] == ["multi", "composite"]
