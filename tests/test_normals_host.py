"""Coloured mesh export without a GPU: the two entries are declared, bound and exported and refuse bad arguments ahead of any launch (dummy
pointers, as in tests/test_kernel_tables.py); the float64 statement of the density gradient (tests/normals_reference.py) against float64 central
differences; the PLY writer's bytes and the attribute reader."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from palettenerf_amd import _lib, mesh
from tests import normals_reference as nref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OK, INVALID, UNSUPPORTED = 0, -1, -2
P = 64      # a non-null, 16-byte aligned address that is never read


def test_entries_are_declared_bound_and_exported_and_the_abi_is_10():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("pnr_density_gradient", "pnr_mesh_vertex_records", "pnr_mesh_vertex_record_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pnr_abi_version() == 10
    assert lib.pnr_mesh_vertex_record_bytes(0, 0, 0) == 12 and lib.pnr_mesh_vertex_record_bytes(1, 0, 0) == 24
    assert lib.pnr_mesh_vertex_record_bytes(1, 1, 17) == 12 + 12 + 4 + 4 * 17 and lib.pnr_mesh_vertex_record_bytes(0, 1, 33) == 12 + 4 + 4 * 33


def test_ctypes_mirrors_have_the_layout_gcc_gives_the_header_structs(tmp_path):
    pairs = {"pnr_density_gradient_args": _lib.DensityGradientArgs, "pnr_vertex_records_args": _lib.VertexRecordsArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {']
    for cname, mirror in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, *_ in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    for cname, mirror in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for fname, *_ in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, f"{cname}.{fname}"
        body = re.sub(r"\[[^\]]*\]", "", re.search(r"typedef struct(?: \w+)? \{([^}]*)\} " + cname + ";", hdr).group(1))
        assert sum(len(decl.split(",")) for decl in body.split(";") if decl.strip()) == len(mirror._fields_), cname


def gradient_args(**over):
    a = _lib.DensityGradientArgs()
    a.points, a.n, a.bound = P, 8, 1.0
    a.embeddings, a.offsets, a.num_levels, a.S, a.base_resolution, a.gridtype = P, P, 16, 0.4666, 16, 0
    a.sigma0, a.sigma1, a.logit, a.grad, a.normal = P, P, P, P, P
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_density_gradient_validates_before_any_launch():
    fn = _lib.load().pnr_density_gradient
    assert fn(None, None) == INVALID
    for over in ({"num_levels": 8}, {"num_levels": 17}, {"gridtype": 2}, {"bound": 0.0}, {"bound": -1.0}, {"bound": float("nan")}):
        assert fn(ctypes.byref(gradient_args(**over)), None) == UNSUPPORTED, over
    for name in ("embeddings", "offsets", "sigma0", "sigma1", "points"):
        assert fn(ctypes.byref(gradient_args(**{name: None})), None) == INVALID, name
    assert fn(ctypes.byref(gradient_args(logit=None, grad=None, normal=None)), None) == INVALID          # nothing asked
    assert fn(ctypes.byref(gradient_args(n=0)), None) == OK
    assert fn(ctypes.byref(gradient_args(n=0, points=None, grad=None, normal=None)), None) == OK           # an empty batch needs no points
    assert fn(ctypes.byref(gradient_args(n=0, logit=None, grad=None, normal=None)), None) == INVALID      # ... but an output


def record_args(**over):
    a = _lib.VertexRecordsArgs()
    a.vertices, a.nv = P, 8
    for d in range(3):
        a.box_min[d], a.box_max[d], a.n[d] = -1.0, 1.0, 33
    a.world, a.records = P, P
    for k, v in over.items():
        if k == "n":
            for d in range(3):
                a.n[d] = v[d]
        else:
            setattr(a, k, v)
    return a


def test_vertex_records_validates_before_any_launch():
    fn = _lib.load().pnr_mesh_vertex_records
    assert fn(None, None) == INVALID
    assert fn(ctypes.byref(record_args(world=None, records=None)), None) == INVALID
    assert fn(ctypes.byref(record_args(n=(33, 1, 33))), None) == INVALID
    assert fn(ctypes.byref(record_args(extra_channels=17, extra_stride=17)), None) == INVALID              # channels without the array
    assert fn(ctypes.byref(record_args(extra=P, extra_channels=17, extra_stride=16)), None) == INVALID
    assert fn(ctypes.byref(record_args(records=P + 2)), None) == INVALID                                   # not 4-byte aligned
    assert fn(ctypes.byref(record_args(vertices=None)), None) == INVALID
    assert fn(ctypes.byref(record_args(nv=0)), None) == OK
    assert fn(ctypes.byref(record_args(nv=0, vertices=None)), None) == OK
    assert fn(ctypes.byref(record_args(nv=1 << 31)), None) == UNSUPPORTED                                  # 3 * 2^31 words
    assert fn(ctypes.byref(record_args(nv=1 << 27, extra=P, extra_channels=33, extra_stride=33, normal=P, rgb=P)), None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ the float64 statement
PLS = float(np.exp2(np.log2(2048 / 16) / 15))


def small_field(gridtype, bound, seed):
    rng = np.random.default_rng(seed)
    offsets = oracle.grid_offsets(3, 16, PLS, 16, 14)
    table = ((rng.random((int(offsets[-1]), 2)) * 2 - 1) * 0.5).astype(np.float32)
    s0 = ((rng.random((64, 32)) * 2 - 1) / np.sqrt(32)).astype(np.float32)
    s1 = ((rng.random((16, 64)) * 2 - 1) / np.sqrt(64)).astype(np.float32)
    return nref.DensityField(table, offsets, PLS, 16, gridtype, s0, s1, bound)


@pytest.mark.parametrize("gridtype,bound", [(0, 1.0), (1, 2.0)], ids=["hash-bound1", "tiled-bound2"])
def test_the_float64_gradient_equals_float64_central_differences(gridtype, bound):
    """Within a cell the encoder is multilinear and sigma_net piecewise linear: along one axis logit is LINEAR while no level leaves its cell and no
    hidden unit crosses its kink, so the central difference quotient is the derivative up to rounding.  The step: 1 % of the finest level's cell."""
    field = small_field(gridtype, bound, 7 + gridtype)
    rng = np.random.default_rng(11)
    pts = ((rng.random((6000, 3)) * 2 - 1) * bound).astype(np.float32)
    x01 = nref.unit_cube(pts, bound)
    geo = nref.RealPositionGeometry(x01, field.offsets, field.per_level_scale, field.base_resolution, field.gridtype, False)
    frac = geo.f[:, :, 1, :]                                                   # [L, D, B]
    keep = ((frac > 0.03) & (frac < 0.97)).all(axis=(0, 1)) & geo.inr
    assert keep.sum() >= 100
    pts, x01 = pts[keep], x01[keep]
    geo = nref.RealPositionGeometry(x01, field.offsets, field.per_level_scale, field.base_resolution, field.gridtype, False)
    x64 = x01.astype(np.float64)
    base = field.evaluate(None, nref.set_positions(geo, x64))
    h = 0.01 / float(geo.scale[-1])
    live = np.ones(len(pts), bool)
    fd = np.zeros((len(pts), 3))
    for d in range(3):
        step = np.zeros(3)
        step[d] = h
        up = field.evaluate(None, nref.set_positions(geo, x64 + step))
        up = {k: v.copy() for k, v in up.items()}
        dn = field.evaluate(None, nref.set_positions(geo, x64 - step))
        live &= ((up["z"] > 0) == (base["z"] > 0)).all(axis=1) & ((dn["z"] > 0) == (base["z"] > 0)).all(axis=1)
        fd[:, d] = (up["logit"] - dn["logit"]) / (2 * h * 2 * bound)           # d / d p = d / d x / (2 bound)
    assert live.sum() >= 50
    g = base["grad"][live]
    err = np.abs(fd[live] - g).max()
    print("rows", int(live.sum()), "max |grad|", float(np.abs(g).max()), "max error", float(err))
    assert np.abs(g).max() > 1.0                                               # a field with a gradient
    assert err <= 1e-8 * np.abs(g).max()
    # the normal is the negated unit gradient
    assert np.allclose(np.linalg.norm(base["normal"][live], axis=1), 1.0, atol=1e-12)
    assert (np.einsum("ij,ij->i", base["normal"][live], g) < 0).all()


def test_points_outside_the_box_read_zero():
    field = small_field(0, 1.0, 3)
    pts = np.array([[1.5, 0, 0], [0, -1.0000001, 0], [0.2, 0.3, 2.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]], np.float32)
    out = field.evaluate(pts)
    assert list(out["inside"]) == [False, False, False, True, True]
    assert (out["logit"][:3] == 0).all() and (out["grad"][:3] == 0).all() and (out["normal"][:3] == 0).all()
    assert (out["grad"][3:] != 0).any(axis=1).all()


# ------------------------------------------------------------------------------------------ PLY
def test_write_ply_without_the_new_arguments_writes_todays_bytes(tmp_path):
    v = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5], [0.1, 0.2, 0.3], [4.0, 5.0, 6.0]], np.float64)
    t = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    path = str(tmp_path / "plain.ply")
    mesh.write_ply(path, v, t)
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            b"element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    want += v.astype("<f4").tobytes()
    for tri in t:
        want += b"\x03" + tri.astype("<i4").tobytes()
    assert open(path, "rb").read() == want
    vr, tr = mesh.read_ply(path)
    assert np.array_equal(vr, v.astype(np.float32)) and np.array_equal(tr, t)
    attrs, comments = mesh.read_ply_attributes(path)
    assert comments == [] and sorted(attrs) == ["triangles", "x", "y", "z"] and np.array_equal(attrs["triangles"], t)


@pytest.mark.parametrize("channels", [0, 17], ids=["color", "palette"])
def test_ply_round_trip_with_records(tmp_path, channels):
    rng = np.random.default_rng(5)
    nv = 9
    lattice = (rng.random((nv, 3)) * 32).astype(np.float32)
    normal = rng.standard_normal((nv, 3)).astype(np.float32)
    rgb = (rng.random((nv, 3)) * 1.4 - 0.2).astype(np.float32)                 # some values outside [0, 1]
    extra = rng.standard_normal((nv, channels)).astype(np.float32)
    world, records = nref.vertex_records(lattice, [-1, -1, -1], [1, 1, 1], (33, 33, 33), normal, rgb, False, extra)
    assert records.shape == (nv, 28 + 4 * channels) and records.dtype == np.uint8
    t = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    props = mesh.XYZ_PROPERTIES + mesh.NORMAL_PROPERTIES + mesh.RGBA_PROPERTIES + (mesh.palette_properties(4) if channels else ())
    comments = ["palette 0 0.25 0.5 0.75", "made by a test"]
    path = str(tmp_path / "coloured.ply")
    mesh.write_ply(path, None, t, records=records, properties=props, comments=comments)
    attrs, got_comments = mesh.read_ply_attributes(path)
    assert got_comments == comments
    assert np.array_equal(np.stack([attrs["x"], attrs["y"], attrs["z"]], 1).view(np.uint32), world.view(np.uint32))
    assert np.array_equal(np.stack([attrs["nx"], attrs["ny"], attrs["nz"]], 1).view(np.uint32), normal.view(np.uint32))
    rgba = np.stack([attrs["red"], attrs["green"], attrs["blue"], attrs["alpha"]], 1)
    assert rgba.dtype == np.uint8 and (rgba[:, 3] == 255).all()
    assert np.array_equal(rgba[:, :3], (np.clip(rgb, 0, 1) * np.float32(255)).astype(np.int32).astype(np.uint8))
    if channels:
        names = [n for _, n in mesh.palette_properties(4)]
        assert names[:6] == ["radiance", "omega_0", "omega_1", "omega_2", "omega_3", "offset_0_r"] and names[-1] == "offset_3_b" and len(names) == 17
        assert np.array_equal(np.stack([attrs[n] for n in names], 1).view(np.uint32), extra.view(np.uint32))
    assert np.array_equal(attrs["triangles"], t)
    vr, tr = mesh.read_ply(path)                                               # the plain reader: x y z and faces of the new file
    assert np.array_equal(vr.view(np.uint32), world.view(np.uint32)) and np.array_equal(tr, t)
    with pytest.raises(ValueError):
        mesh.write_ply(path, None, t, records=records[:, :-1], properties=props)
