"""Coloured mesh export on the GPU: pnr_density_gradient against the float64 statement of tests/normals_reference.py with the per-op (autograd)
formulation as the fp32 yardstick, its bits under permutation / chunking / repetition, the fallback for other fields, pnr_mesh_vertex_records
against the numpy statement byte for byte, the sign convention of the normals against the triangles' winding, and save_mesh end to end.

pnr_density_gradient launches ceil(n / 256) workgroups whatever n is: there is no capped grid and no tile loop, so no row takes a second trip
(pnr_launch_geometry does not know the entry; asserted below)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, mesh, network, rays, renderer, scene
from palettenerf_amd.encoding import get_encoder
from tests import normals_reference as nref

pytestmark = pytest.mark.gpu

N = 4099
FIELDS = [(1, "hashgrid"), (2, "hashgrid"), (1, "tiledgrid"), (2, "tiledgrid")]
FIELD_IDS = [f"bound{b}-{e[:-4]}" for b, e in FIELDS]


def shipped_model(cuda, bound=1, encoding="hashgrid"):
    m = scene.seed_field_(network.NeRFNetwork(encoding=encoding, bound=bound, cuda_ray=True), 0)
    return m.to(cuda).eval()


@functools.lru_cache(maxsize=None)
def sample_points(bound):
    """[4099, 3] fp32: uniform in the box, then 96 outside it, 54 on its faces, the 8 corners and the centre."""
    rng = np.random.default_rng(40 + bound)
    p = ((rng.random((N, 3)) * 2 - 1) * bound).astype(np.float32)
    out = p[3900:3996]
    axis = rng.integers(0, 3, len(out))
    out[np.arange(len(out)), axis] = (np.where(rng.random(len(out)) < 0.5, -1, 1) * bound * (1 + rng.random(len(out)))).astype(np.float32)
    out[0, 0] = np.nextafter(np.float32(bound), np.float32(np.inf))                       # one ulp outside
    out[1, 1] = -np.nextafter(np.float32(bound), np.float32(np.inf))
    out[2] = 1.0e6
    face = p[3996:4050]
    axis = rng.integers(0, 3, len(face))
    face[np.arange(len(face)), axis] = np.where(rng.random(len(face)) < 0.5, -bound, bound)
    p[4050:4058] = np.array([[x, y, z] for x in (-bound, bound) for y in (-bound, bound) for z in (-bound, bound)], np.float32)
    p[4058] = 0.0
    p.setflags(write=False)
    return p


_cases = {}


def case(cuda, bound, encoding):
    """Per field, computed once and shared: the model, the points, the float64 statement, the ambiguous rows, the per-op yardstick and its errors E."""
    key = (bound, encoding)
    if key not in _cases:
        m = shipped_model(cuda, bound, encoding)
        assert m._fused_sweep_ok()
        p = sample_points(bound)
        f64 = nref.DensityField.of_model(m).evaluate(p)
        # (a row outside the box is not ambiguous: its features, and with them every pre-activation, are exactly zero in fp32 and float64 alike)
        amb = nref.ambiguous_rows(f64["enc"], m.sigma_net[0].weight.detach().cpu().numpy(), margin=2e-5) & f64["inside"]
        pts = torch.from_numpy(p.copy()).to(cuda)
        per_op = {k: v.cpu().numpy().astype(np.float64) for k, v in mesh.density_gradient_per_op(m, pts).items()}
        rows = ~amb
        E_grad = float(np.abs(per_op["grad"] - f64["grad"])[rows].max())
        E_sigma = float(np.abs(per_op["sigma"] - np.exp(f64["logit"]))[rows].max())
        for a in f64.values():
            a.setflags(write=False)
        _cases[key] = dict(model=m, p=p, pts=pts, f64=f64, amb=amb, rows=rows, per_op=per_op, E_grad=E_grad, E_sigma=E_sigma)
    return _cases[key]


@pytest.mark.parametrize("bound,encoding", FIELDS, ids=FIELD_IDS)
def test_gradient_and_density_against_float64_with_the_per_op_path_as_yardstick(cuda, bound, encoding):
    """Tolerance 4 E, E = the max-norm error of density_gradient_per_op (fp32 autograd) against the same float64 statement on the same rows.  Rows with a
    hidden unit within 2e-5 of the ReLU's kink (float64) may fall either way in fp32: finiteness only, and at most 3 % of the rows."""
    c = case(cuda, bound, encoding)
    f64, rows, amb = c["f64"], c["rows"], c["amb"]
    print("ambiguous share", float(amb.mean()), "inside", int(f64["inside"].sum()))
    assert amb.mean() <= 0.03
    assert 4000 <= f64["inside"].sum() < N                                                  # both kinds of rows occur
    got = mesh.density_gradient(c["model"], c["pts"])
    assert sorted(got) == ["grad", "normal", "sigma"] and all(v.is_cuda and v.dtype == torch.float32 for v in got.values())
    grad, sigma = got["grad"].cpu().numpy().astype(np.float64), got["sigma"].cpu().numpy().astype(np.float64)
    assert np.isfinite(grad).all() and np.isfinite(sigma).all() and np.isfinite(got["normal"].cpu().numpy()).all()
    err_grad = float(np.abs(grad - f64["grad"])[rows].max())
    err_sigma = float(np.abs(sigma - np.exp(f64["logit"]))[rows].max())
    print(f"max |grad| {np.abs(f64['grad']).max():.4g}  E_grad (per-op) {c['E_grad']:.4g}  kernel {err_grad:.4g}   "
          f"E_sigma (per-op) {c['E_sigma']:.4g}  kernel {err_sigma:.4g}")
    assert c["E_grad"] > 0 and c["E_sigma"] > 0
    assert err_grad <= 4 * c["E_grad"]
    assert err_sigma <= 4 * c["E_sigma"]
    # the two formulations against each other, on the shipped model
    assert np.abs(grad - c["per_op"]["grad"])[rows].max() <= 4 * c["E_grad"]
    assert np.abs(sigma - c["per_op"]["sigma"])[rows].max() <= 4 * c["E_sigma"]
    # outside the box the encoder reads zero
    outside = ~f64["inside"]
    assert (grad[outside] == 0).all() and (sigma[outside] == 1).all()


@pytest.mark.parametrize("bound,encoding", FIELDS, ids=FIELD_IDS)
def test_normals_are_the_negated_unit_gradient(cuda, bound, encoding):
    """|normal - (-g / |g|)| <= 2 tol_grad / |g| + 4 * 2^-24: normalising moves a vector by at most twice its relative error, and the kernel's own
    normalisation (an exact power-of-two scaling, three products, two sums, a root, a quotient) rounds each component by less than 4 units."""
    c = case(cuda, bound, encoding)
    f64 = c["f64"]
    tol = 4 * c["E_grad"]
    normal = mesh.density_gradient(c["model"], c["pts"], want=("normal",))["normal"].cpu().numpy().astype(np.float64)
    length = np.linalg.norm(f64["grad"], axis=1)
    sel = c["rows"] & (length > 0)
    assert sel.sum() > 3900
    miss = np.linalg.norm(normal - f64["normal"], axis=1)[sel]
    allowed = 2 * tol / length[sel] + 4 * 2.0 ** -24
    print("worst normal error / allowed", float((miss / allowed).max()), "largest", float(miss.max()))
    assert (miss <= allowed).all()
    assert (normal[~f64["inside"]] == 0).all()
    assert np.abs(np.linalg.norm(normal[f64["inside"] & (length > 0)], axis=1) - 1).max() < 1e-6


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_a_rows_bits_depend_on_the_row_alone(cuda, n):
    c = case(cuda, 1, "hashgrid")
    m = c["model"]
    pts = torch.cat([c["pts"][3890:3890 + n - n // 2], c["pts"][:n // 2]]).contiguous()          # outside rows among them from n = 63 on
    whole = mesh.density_gradient(m, pts)
    again = mesh.density_gradient(m, pts)
    perm = torch.from_numpy(np.random.default_rng(n).permutation(n)).to(cuda)
    shuffled = mesh.density_gradient(m, pts[perm].contiguous())
    for k in ("sigma", "grad", "normal"):
        assert np.array_equal(bits(again[k]), bits(whole[k])), k
        assert np.array_equal(bits(shuffled[k]), bits(whole[k][perm])), k
        alone = mesh.density_gradient(m, pts, want=(k,))
        assert list(alone) == [k] and np.array_equal(bits(alone[k]), bits(whole[k])), k
    if n > 1:
        h = n // 2
        a, b = mesh.density_gradient(m, pts[:h].contiguous()), mesh.density_gradient(m, pts[h:].contiguous())
        for k in ("sigma", "grad", "normal"):
            assert np.array_equal(np.concatenate([bits(a[k]), bits(b[k])]), bits(whole[k])), k


def test_the_entry_has_no_capped_grid_and_an_empty_batch_is_empty(cuda):
    with pytest.raises(RuntimeError):
        _lib.launch_geometry("pnr_density_gradient", 1 << 20)
    m = case(cuda, 1, "hashgrid")["model"]
    out = mesh.density_gradient(m, torch.empty(0, 3, device=cuda))
    assert tuple(out["sigma"].shape) == (0,) and tuple(out["grad"].shape) == (0, 3) and tuple(out["normal"].shape) == (0, 3)


def test_other_fields_take_the_per_op_path(cuda, monkeypatch):
    def no_kernel(*a, **k):
        raise AssertionError("the fused kernel was launched for a field it does not evaluate")

    pts = case(cuda, 1, "hashgrid")["pts"][:300]
    # eight levels: another architecture
    m8 = network.NeRFNetwork(bound=1, cuda_ray=True)
    m8.encoder, m8.in_dim = get_encoder("hashgrid", num_levels=8, desired_resolution=2048)
    m8.sigma_net = network._mlp([m8.in_dim, 64, 16])
    m8 = scene.seed_field_(m8, 1).to(cuda).eval()
    assert m8.encoder.num_levels == 8 and not m8._fused_sweep_ok()
    shipped = case(cuda, 1, "hashgrid")["model"]
    fused = mesh.density_gradient(shipped, pts)
    monkeypatch.setattr(mesh, "_density_gradient_fused", no_kernel)
    out = mesh.density_gradient(m8, pts)
    want = mesh.density_gradient_per_op(m8, pts)
    for k in ("sigma", "grad", "normal"):
        assert torch.isfinite(out[k]).all() and torch.allclose(out[k], want[k], rtol=1e-5, atol=1e-6), k
    inside = (pts.abs() <= 1).all(dim=1)
    assert torch.allclose(out["normal"][inside].norm(dim=1), torch.ones(int(inside.sum()), device=cuda), atol=1e-5)
    # a density() replaced on the instance is asked, not bypassed
    m = shipped_model(cuda)
    calls = []

    def density(x):
        calls.append(x.shape[0])
        return type(m).density(m, x)

    m.density = density
    assert not m._fused_sweep_ok()
    out = mesh.density_gradient(m, pts)
    assert calls == [300]
    c = case(cuda, 1, "hashgrid")
    rows = torch.from_numpy(c["rows"][:300]).to(cuda)
    assert (out["grad"] - fused["grad"])[rows].abs().max() <= 4 * c["E_grad"]
    assert (out["sigma"] - fused["sigma"])[rows].abs().max() <= 4 * c["E_sigma"]


# ------------------------------------------------------------------------------------------ vertex records
LO, HI, RES = (-1.25, 0.1, -3.0), (0.75, 0.9, 5.5), (33, 20, 257)
COMBOS = [  # normal, rgb, sRGB, extra channels
    (False, False, False, 0), (True, False, False, 0), (False, True, False, 0), (True, True, False, 0), (True, True, True, 0),
    (True, True, False, 17), (True, True, True, 33), (False, False, False, 33), (False, True, True, 17)]


@pytest.mark.parametrize("nv", [0, 1, 255, 257])
def test_vertex_records_equal_the_numpy_statement_byte_for_byte(cuda, nv):
    rng = np.random.default_rng(nv)
    v = (rng.random((nv, 3)) * (np.asarray(RES) - 1)).astype(np.float32)
    if nv:
        v[0] = 0
        v[-1] = np.asarray(RES, np.float32) - 1                                              # the box's own corners
    normal = rng.standard_normal((nv, 3)).astype(np.float32)
    rgb = (rng.random((nv, 3)) * 1.5 - 0.25).astype(np.float32)                               # a third outside [0, 1]
    if nv > 2:
        rgb[1] = [np.nan, 0.0, 1.0]
        rgb[2] = [0.0031308, 0.003, 0.5]
    extra33 = rng.standard_normal((nv, 33)).astype(np.float32)
    vd = torch.from_numpy(v).to(cuda)
    want_world = nref.world_vertices(v, LO, HI, RES).astype(np.float32)                       # extract_geometry's float64 vertices, rounded once
    for with_normal, with_rgb, srgb, channels in COMBOS:
        extra = extra33[:, :channels]
        world, rec = mesh.vertex_records(vd, LO, HI, RES, normal=torch.from_numpy(normal).to(cuda) if with_normal else None,
                                         rgb=torch.from_numpy(rgb).to(cuda) if with_rgb else None,
                                         extra=torch.from_numpy(np.ascontiguousarray(extra)).to(cuda) if channels else None, linear_to_srgb=srgb)
        _, want = nref.vertex_records(v, LO, HI, RES, normal if with_normal else None, rgb if with_rgb else None, srgb, extra if channels else None)
        rec = rec.cpu().numpy()
        assert rec.shape == want.shape == (nv, 12 + 12 * with_normal + 4 * with_rgb + 4 * channels)
        assert np.array_equal(world.cpu().numpy().view(np.uint32), want_world.view(np.uint32))
        if with_rgb and srgb and nv:
            # the curve's powf is the device library's: the bytes are pnr_image_to_uint8's on the clipped colour, and within one of numpy's
            at = 12 + 12 * with_normal
            dev = rays.image_to_uint8(torch.nan_to_num(torch.from_numpy(rgb).to(cuda), nan=0.0).clamp(0, 1), True).cpu().numpy()
            assert np.array_equal(rec[:, at:at + 3], dev)
            assert np.abs(rec[:, at:at + 3].astype(int) - want[:, at:at + 3].astype(int)).max() <= 1
            want[:, at:at + 3] = dev
        assert np.array_equal(rec, want), (with_normal, with_rgb, srgb, channels)
    if nv:
        # rows of `extra` wider than the channels written, world alone, records alone: through the C ABI
        wide = torch.from_numpy(extra33).to(cuda)
        rec = torch.zeros(nv, 12 + 4 * 17, dtype=torch.uint8, device=cuda)
        a = _lib.VertexRecordsArgs()
        a.vertices, a.nv = vd.data_ptr(), nv
        for d in range(3):
            a.box_min[d], a.box_max[d], a.n[d] = LO[d], HI[d], RES[d]
        a.extra, a.extra_channels, a.extra_stride, a.records = wide.data_ptr(), 17, 33, rec.data_ptr()
        _lib.check(_lib.load().pnr_mesh_vertex_records(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "records")
        assert np.array_equal(rec.cpu().numpy(), nref.vertex_records(v, LO, HI, RES, extra=extra33[:, :17])[1])
        world, none = mesh.vertex_records(vd, LO, HI, RES, want_records=False)
        assert none is None and np.array_equal(world.cpu().numpy().view(np.uint32), want_world.view(np.uint32))


# ------------------------------------------------------------------------------------------ orientation
def test_normals_point_to_the_side_the_triangles_are_counter_clockwise_from(cuda):
    """A smooth field (the coarsest level alone), meshed at R = 33 at the volume's median.  A face normal (b - a) x (c - a) of a counter-clockwise
    triangle points to the low-density side, and so does -grad: the two agree in sign on most triangles and in the area-weighted sum.  A flipped
    convention on either side gives the negative of both figures."""
    m = shipped_model(cuda)
    with torch.no_grad():
        m.encoder.embeddings[int(m.encoder.offsets[1]):] = 0
    R = 33
    u = mesh.lattice_density(m, resolution=R)
    thr = float(u.median())
    v, t = mesh.marching_cubes(u, thr)
    assert t.shape[0] > 500
    world, _ = mesh.vertex_records(v, m.aabb_infer[:3], m.aabb_infer[3:], R, want_records=False)
    n = mesh.density_gradient(m, world, want=("normal",))["normal"].cpu().numpy().astype(np.float64)
    w, t = world.cpu().numpy().astype(np.float64), t.cpu().numpy()
    a, b, c = (w[t[:, k]] for k in range(3))
    face = np.cross(b - a, c - a)                                                            # length = twice the area
    area = np.linalg.norm(face, axis=1)
    unit = face / np.where(area > 0, area, 1)[:, None]
    dots = np.einsum("ij,ij->i", unit, n[t].mean(axis=1))
    print("triangles", len(t), "agreeing share", float((dots > 0).mean()), "area-weighted sum", float((dots * area).sum()))
    assert (dots > 0).mean() > 0.5
    assert (dots * area).sum() > 0


# ------------------------------------------------------------------------------------------ end to end
def median_threshold(m, R):
    return float(mesh.lattice_density(m, resolution=R).median())


def view_dirs(normal):
    up = torch.zeros_like(normal)
    up[:, 2] = 1
    return torch.where((normal == 0).all(dim=1, keepdim=True), up, -normal).contiguous()


def test_a_palette_model_from_field_to_recolourable_ply(cuda, tmp_path):
    R, nb = 33, 4
    m = scene.seed_field_(network.PaletteNetwork(renderer.default_opt(num_basis=nb), bound=1, cuda_ray=True), 0).to(cuda).eval()
    with torch.no_grad():
        m.basis_color[0, 0], m.basis_color[1, 1] = 1.3, -0.2                                 # a palette that needs its clamp
    thr = median_threshold(m, R)
    # attributes=None: the parent's file, byte for byte
    plain, parent = str(tmp_path / "plain.ply"), str(tmp_path / "parent.ply")
    v0, t0 = mesh.save_mesh(m, plain, resolution=R, threshold=thr)
    pv, pt = mesh.extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], R, thr, model=m)
    mesh.write_ply(parent, pv, pt)
    assert open(plain, "rb").read() == open(parent, "rb").read() and len(pt) > 500
    assert np.array_equal(v0, pv) and np.array_equal(t0, pt)
    # attributes="palette"
    path = str(tmp_path / "palette.ply")
    v, t, attrs = mesh.save_mesh(m, path, resolution=R, threshold=thr, attributes="palette")
    assert v.dtype == np.float64 and np.array_equal(v, pv) and np.array_equal(t, pt)
    got, comments = mesh.read_ply_attributes(path)
    xyz = np.stack([got["x"], got["y"], got["z"]], 1)
    plain_v, plain_t = mesh.read_ply(plain)
    assert np.array_equal(xyz.view(np.uint32), plain_v.view(np.uint32)) and np.array_equal(got["triangles"], plain_t)
    rv, rt = mesh.read_ply(path)
    assert np.array_equal(rv.view(np.uint32), plain_v.view(np.uint32)) and np.array_equal(rt, plain_t)
    world = torch.from_numpy(plain_v).to(cuda)
    want = mesh.vertex_attributes(m, world)
    assert sorted(want) == sorted(["normal", "diffuse", "view_dep", "omega", "radiance", "offsets", "base_rgb", "rgb"])
    for k in want:
        assert np.array_equal(bits(want[k]), bits(attrs[k])), k
    nv = len(plain_v)
    # in chunks with a ragged last one: the same rows (the normals bit for bit: a row's gradient depends on the row alone; the model's own forward
    # may pick other library kernels for another batch size, so its outputs are held to fp32 rounding)
    chunked = mesh.vertex_attributes(m, world, chunk=nv // 3 + 1)
    assert sorted(chunked) == sorted(want) and np.array_equal(bits(chunked["normal"]), bits(want["normal"]))
    for k in want:
        assert chunked[k].shape == want[k].shape and torch.allclose(chunked[k], want[k], rtol=1e-5, atol=1e-6), k
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], 1).view(np.uint32), bits(want["normal"]))
    names = [n for _, n in mesh.palette_properties(nb)]
    floats = np.stack([got[n] for n in names], 1)
    assert floats.shape == (nv, 17)
    assert np.array_equal(floats[:, 0].view(np.uint32), bits(want["radiance"]))
    assert np.array_equal(floats[:, 1:1 + nb].view(np.uint32), bits(want["omega"]))
    assert np.array_equal(floats[:, 1 + nb:].view(np.uint32), bits(want["offsets"]).reshape(nv, 3 * nb))
    rgba = np.stack([got["red"], got["green"], got["blue"], got["alpha"]], 1)
    # pnr_image_to_uint8 does not clip (its callers do): the record's rule is clip, then its expression
    assert np.array_equal(rgba[:, :3], rays.image_to_uint8(want["base_rgb"].clamp(0, 1)).cpu().numpy()) and (rgba[:, 3] == 255).all()
    assert len(np.unique(rgba[:, :3], axis=0)) > 50
    # the palette, clamped, in the comments
    palette = m.basis_color.detach().float().clamp(0, 1).cpu().numpy()
    assert len(comments) == nb and palette.max() == 1.0 and palette.min() == 0.0
    parsed = np.array([[float(x) for x in c.split()[2:]] for c in comments])
    assert [c.split()[:2] for c in comments] == [["palette", str(b)] for b in range(nb)]
    assert np.array_equal(parsed.astype(np.float32), palette)
    # base_rgb from what the file carries: float64 against the exported value, the fp32 torch expression as yardstick
    omega, radiance, offsets = floats[:, 1:1 + nb], floats[:, 0], floats[:, 1 + nb:].reshape(nv, nb, 3)

    def compose(dtype):
        o, r, f, p = (torch.from_numpy(np.ascontiguousarray(x)).to(dtype) for x in (omega, radiance, offsets, parsed.astype(np.float32)))
        return (o[:, :, None] * (r[:, None, None] * (p[None] + f))).sum(dim=-2)

    exact = compose(torch.float64)
    yard = float((compose(torch.float32).double() - exact).abs().max())
    miss = float((want["base_rgb"].cpu().double() - exact).abs().max())
    print("vertices", nv, "base_rgb: fp32 torch expression", yard, "exported", miss)
    assert yard > 0 and miss <= 4 * yard
    assert torch.equal(want["rgb"], want["base_rgb"] + want["view_dep"])
    # attributes="color" on the same model: normals and base_rgb, nothing else
    col = str(tmp_path / "color.ply")
    mesh.save_mesh(m, col, resolution=R, threshold=thr, attributes="color", linear_to_srgb=True)
    got_c, comments_c = mesh.read_ply_attributes(col)
    assert comments_c == [] and sorted(got_c) == sorted(["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha", "triangles"])
    assert np.array_equal(np.stack([got_c["red"], got_c["green"], got_c["blue"]], 1),
                          rays.image_to_uint8(want["base_rgb"].clamp(0, 1), True).cpu().numpy())


def test_a_nerf_model_exports_colour_and_refuses_a_palette(cuda, tmp_path):
    R = 33
    m = shipped_model(cuda)
    thr = median_threshold(m, R)
    path = str(tmp_path / "meshes" / "nerf.ply")
    v, t, attrs = mesh.save_mesh(m, path, resolution=R, threshold=thr, attributes="color")
    assert sorted(attrs) == ["normal", "rgb"] and len(t) > 500
    got, comments = mesh.read_ply_attributes(path)
    assert comments == []
    xyz = np.stack([got["x"], got["y"], got["z"]], 1)
    assert np.array_equal(xyz, v.astype(np.float32)) and np.array_equal(got["triangles"], t)
    x = torch.from_numpy(xyz).to(cuda)
    normal = mesh.density_gradient(m, x, want=("normal",))["normal"]
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], 1).view(np.uint32), bits(normal))
    with torch.no_grad():
        rgb = m(x, view_dirs(normal))[1]
    rgba = np.stack([got["red"], got["green"], got["blue"], got["alpha"]], 1)
    assert np.array_equal(rgba[:, :3], rays.image_to_uint8(rgb).cpu().numpy()) and (rgba[:, 3] == 255).all()
    with pytest.raises(ValueError):
        mesh.save_mesh(m, str(tmp_path / "no.ply"), resolution=R, threshold=thr, attributes="palette")
    with pytest.raises(ValueError):
        mesh.save_mesh(m, str(tmp_path / "no.ply"), resolution=R, threshold=thr, attributes="colour")
    # an empty surface is a valid coloured file
    v, t, attrs = mesh.save_mesh(m, path, resolution=R, threshold=1e30, attributes="color")
    got, _ = mesh.read_ply_attributes(path)
    assert len(v) == 0 and len(t) == 0 and len(got["x"]) == 0 and got["red"].dtype == np.uint8 and tuple(attrs["rgb"].shape) == (0, 3)
