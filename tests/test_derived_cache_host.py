"""The cache of everything the fused objects derive from parameters (fused._Derived) and the state declared next to it (fused._FusedState), on CPU
tensors and CPU models: no device needed."""
import copy
import pathlib
import pickle
import re
import warnings

import pytest
import torch

from palettenerf_amd import fused, network

STATE_AT_START = dict(_gen=0, _slot=1, _handed=None, _overflowed_key=None, _watch_keys=None, _watch_ref=None, _watch_dev=None, _watch_host=None, _watch_rows=None,
                      _guard_hold=False, _guard_held=None, _weights_held=None, _ws=None, ray_order=None, time_grid_kernel=False)


class Owner:
    def __init__(self):
        self.cache = fused._Derived()
        self.name = "owner"


def test_the_cache_alone(monkeypatch):
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    built = []

    def build(t):
        built.append(1)
        return t * 2.0

    o = Owner()
    c = o.cache
    assert c.peek("blob") is None and c.key("blob") is None and c.slots() == []
    v0 = c.get("blob", fused._pkey(src), build, src)
    assert len(built) == 1 and c.peek("blob") is v0 and c.key("blob") == fused._pkey(src) and c.slots() == ["blob"]
    assert c.get("blob", fused._pkey(src), build, src) is v0 and len(built) == 1          # same key: the same object, build is not called
    before = v0.clone()
    src.add_(1.0)                                                                           # an in-place op bumps the version
    v1 = c.get("blob", fused._pkey(src), build, src)
    assert len(built) == 2 and v1 is not v0 and c.peek("blob") is v1
    assert torch.equal(v0, before) and torch.equal(v1, src * 2.0)                           # the value handed out earlier is as it was
    other = c.get(("blob", 1), "k", build, src)                                             # slots are independent of each other
    assert other is not v1 and c.peek("blob") is v1 and set(c.slots()) == {"blob", ("blob", 1)}

    for dup in (copy.deepcopy(o), pickle.loads(pickle.dumps(o))):                           # a copy of the owner carries no values along
        assert dup.name == "owner" and dup.cache is not c and dup.cache.slots() == [] and dup.cache.peek("blob") is None
    assert c.peek("blob") is v1

    moved = fused._pkey(torch.zeros(1))                                                     # drop: the slots whose key holds a source key, at any depth
    c.get("deep", ("x", 1.0, None, (fused._pkey(src), (moved, 2))), list)
    c.get("flat", moved, list)
    c.drop({moved})
    assert set(c.slots()) == {"blob", ("blob", 1)} and c.peek("blob") is v1
    c.drop({fused._pkey(src)})
    assert c.slots() == [("blob", 1)]
    c.get("blob", fused._pkey(src), build, src)
    c.clear()
    assert c.slots() == [] and c.peek("blob") is None and c.key("blob") is None and c.key(("blob", 1)) is None
    v2 = c.get("blob", fused._pkey(src), build, src)
    assert len(built) == 5 and v2 is not v1

    monkeypatch.setattr(fused, "PARANOID", True)                                            # every get builds
    v3 = c.get("blob", fused._pkey(src), build, src)
    v4 = c.get("blob", fused._pkey(src), build, src)
    assert len(built) == 7 and v3 is not v2 and v4 is not v3 and torch.equal(v3, v4)


def make(kind):
    if kind == "background":
        m = network.NeRFNetwork(bound=2, cuda_ray=False, bg_radius=4)
        return m, fused.BackgroundFused(m)
    m = network.NeRFNetwork(bound=2, cuda_ray=False)
    return m, (fused.NeRFFieldFused if kind == "nerf" else fused.DensityFused)(m)


@pytest.mark.parametrize("kind", ["nerf", "density", "background"])
def test_a_fresh_object_has_every_state_attribute_at_its_start_value(kind):
    m, f = make(kind)
    for name, start in STATE_AT_START.items():
        assert name in f.__dict__, name
        assert f.__dict__[name] is start or f.__dict__[name] == start, name
    assert isinstance(f._cache, fused._Derived) and f._cache.slots() == []
    assert f.packed is None and f.versions is None
    gen = f._gen
    f._cache.get("blob", 1, list)
    f.invalidate_caches()
    assert f._cache.slots() == [] and f._gen == gen + 1
    dup = copy.deepcopy(f)                                                                  # with its model; the copy's cache is its own and empty
    f._cache.get("blob", 1, list)
    assert dup._cache is not f._cache and dup._cache.slots() == []


@pytest.mark.parametrize("kind", ["nerf", "density"])
def test_guard_slot_follows_the_weights_it_is_computed_from(kind):
    m, f = make(kind)
    calls = []
    bound = type(f)._guard_bound
    f._guard_bound = lambda tmax, scales: (calls.append(1), bound(f, tmax, scales))[1]      # (an instance override, as the GPU tests use one)
    first = f.frame_precision()
    state = f._cache.peek("guard")
    assert first == (1, False) and len(calls) == 1 and state is not None
    assert f.frame_precision() == first and len(calls) == 1 and f._cache.peek("guard") is state      # not rebuilt between two calls
    key = f._cache.key("guard")
    blob_key = lambda: tuple(fused._pkey(t) for t in f._blob_sources())      # (what _pack keys the blob on, next to the device and the precision)
    blob_key0 = blob_key()
    with torch.no_grad():
        m.color_net[0].weight.mul_(1.5)
    f.frame_precision()
    assert (blob_key() == blob_key0) == (kind == "density")
    if kind == "density":        # only sigma_net runs there: a colour-head update rebuilds neither the guard nor the blob key
        assert len(calls) == 1 and f._cache.peek("guard") is state and f._cache.key("guard") == key
        srcs = f._blob_sources()
        assert len(srcs) == 2 and srcs[0] is m.sigma_net[0].weight and srcs[1] is m.sigma_net[1].weight
    else:
        assert len(calls) == 2 and f._cache.peek("guard") is not state
    calls.clear()
    state = f._cache.peek("guard")
    with torch.no_grad():
        m.sigma_net[0].weight.mul_(1.5)
    f.frame_precision()
    assert len(calls) == 1 and f._cache.peek("guard") is not state and f._cache.key("guard") != key


@pytest.mark.parametrize("kind", ["nerf", "density"])
def test_an_overflow_is_remembered_until_a_weight_changes_and_an_invalidation_empties_every_slot(kind):
    m, f = make(kind)
    f._guard_bound = lambda tmax, scales: 1.0e9             # weights that fail the static bound: the frame loops keep split-fp16 and watch
    assert f.frame_precision() == (1, True) and f._gen == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f._note_overflow()
    assert f._gen == 1 and f._overflowed_key is not None and f._overflowed_key == f._cache.key("guard")
    assert f.frame_precision() == (0, False) and f.frame_precision() == (0, False)
    f.invalidate_caches()                                   # the same weights: still remembered once the guard is computed again
    assert f._cache.slots() == [] and f._cache.peek("guard") is None and f._gen == 2
    assert f.frame_precision() == (0, False) and f._cache.slots() == ["guard"]
    with torch.no_grad():
        m.sigma_net[1].weight.mul_(0.5)
    assert f.frame_precision() == (1, True) and f._gen == 2

    f._cache.get("half_table", 0, list)
    f._cache.get(("blob", 1), 0, list)
    f._watch_ref, f._guard_held, f._weights_held = (1,), (2,), [3]
    f.invalidate_caches()
    assert f._cache.slots() == [] and f._gen == 3 and f._watch_ref is None and f._guard_held is None and f._weights_held is None


def test_fused_py_does_not_probe_its_own_private_state():
    """A fence against regrowth: every private attribute of the fused objects is declared by _FusedState._init_state, so the file needs no
    `getattr(self, "_x", None)` and no `self.__dict__.get("_x")`."""
    text = pathlib.Path(fused.__file__).read_text()
    assert re.findall(r"""getattr\(\s*self\s*,\s*["']_""", text) == []
    assert re.findall(r"""self\.__dict__\.get\(\s*["']_""", text) == []
