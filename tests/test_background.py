"""The background model (bg_radius > 0) on the host: parameter names and shapes are the reference's (tests/golden/background_layout.json, checked
against the reference's own modules when it was written), nothing changes without it, and the level layout of the 2-D table is the oracle's."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
from palettenerf_amd import network, renderer
from palettenerf_amd.gridencoder import level_offsets


def layout(golden_dir):
    with open(os.path.join(golden_dir, "background_layout.json")) as f:
        return json.load(f)


def build(kind, **kw):
    if kind == "nerf":
        return network.NeRFNetwork(bound=2, cuda_ray=True, **kw)
    return network.PaletteNetwork(renderer.default_opt(), bound=2, cuda_ray=True, **kw)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
def test_constructor_yields_the_reference_names_and_shapes(golden_dir, kind):
    want = layout(golden_dir)
    plain, m = build(kind).state_dict(), build(kind, bg_radius=4).state_dict()
    added = {k: {"shape": list(v.shape), "dtype": str(v.dtype)} for k, v in m.items() if k not in plain}
    assert added == want["entries"]
    assert m["encoder_bg.offsets"].tolist() == want["offsets"]
    assert set(plain) <= set(m)


@pytest.mark.parametrize("kind", ["nerf", "palette"])
@pytest.mark.parametrize("radius", [-1, 0])
def test_without_a_background_nothing_changes(golden_dir, kind, radius):
    m = build(kind, bg_radius=radius)
    assert m.bg_net is None and not hasattr(m, "encoder_bg")
    assert not any(k.startswith(("encoder_bg", "bg_net")) for k in m.state_dict())
    with open(os.path.join(golden_dir, "state_dict_layout.json")) as f:
        pinned = json.load(f)[kind]        # the reference's own layout of the model without a background
    sd = m.state_dict()
    if kind == "nerf":
        assert {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()} == pinned
    else:
        assert not any(k.startswith(("encoder_bg", "bg_net")) for k in pinned) and set(pinned) - set(sd) <= {"clip_net.0.weight", "clip_net.1.weight"}
    assert list(sd) == list(build(kind).state_dict())


def test_get_params_has_six_groups():
    m = build("nerf", bg_radius=4)
    groups = m.get_params(1e-2)
    assert len(groups) == 6 and len(build("nerf").get_params(1e-2)) == 4
    assert [p.shape for p in groups[4]["params"]] == [m.encoder_bg.embeddings.shape]
    assert [tuple(p.shape) for p in groups[5]["params"]] == [(64, 24), (3, 64)]
    p = build("palette", bg_radius=4)
    assert len(p.get_params(1e-2)) == len(build("palette").get_params(1e-2)) + 2


def test_level_offsets_of_the_2d_table_are_the_oracles(golden_dir):
    pls = np.exp2(np.log2(2048 / 16) / 3)
    ours = level_offsets(2, 4, pls, 16, 19)
    assert np.array_equal(ours, oracle.grid_offsets(2, 4, float(pls), 16, 19))
    assert ours.tolist() == layout(golden_dir)["offsets"]
    e = build("nerf", bg_radius=4).encoder_bg
    assert (e.input_dim, e.num_levels, e.level_dim, e.base_resolution, e.gridtype_id, e.align_corners) == (2, 4, 2, 16, 0, False)
    assert e.offsets.tolist() == ours.tolist()


def test_reference_named_state_dict_with_background_loads_strictly():
    src = build("palette", bg_radius=4)
    sd = {k: torch.randn_like(v) * 0.1 if v.dtype.is_floating_point else v for k, v in src.state_dict().items()}
    dst = build("palette", bg_radius=4)
    dst.load_state_dict(sd)          # strict
    assert torch.equal(dst.bg_net[1].weight, sd["bg_net.1.weight"]) and torch.equal(dst.encoder_bg.embeddings, sd["encoder_bg.embeddings"])
    assert dst.bg_net[0].bias is None and dst.bg_net[1].bias is None
    with pytest.raises(RuntimeError):
        build("palette").load_state_dict(sd)     # a model without the background has no place for them
