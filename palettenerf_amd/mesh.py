"""Mesh export: the tail of the reference's Trainer.save_mesh (nerf/utils.py:187-217, :633-653) on the device.

The reference queries density() on a resolution^3 lattice in blocks built with linspace / meshgrid / cat, reads every block back, runs PyMCubes
on the CPU and lets trimesh write a .ply.  Here the shipped field fills a device volume in one call (pnr_lattice_density: the occupancy sweep's
lookup and sigma_net kernels on lattice points), any other field is handed the points in chunks (pnr_lattice_points) and asked through its own
density(), marching cubes runs over the volume on the device (csrc/mesh.hip: count, one scan, emit) and the host reads back two counts and the
exact-size result.  The vertex and triangle order is fixed (include/pnr.h), so the output is reproducible bit for bit.

Triangles are counter-clockwise seen from the low-density side (normals point out of the dense region).

Beyond the reference: save_mesh(..., attributes="color" | "palette") gives every vertex a normal (density_gradient: pnr_density_gradient, the gradient
of the density's logarithm in one launch for the shipped field, autograd through density() for any other), the model's colour at the view direction
-normal (vertex_attributes) and, for a PaletteNeRF model, its palette weights, offsets and radiance; the vertex block of the file is formed on the
device (vertex_records: pnr_mesh_vertex_records).  Without `attributes` the file is the reference's, byte for byte.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._torch_glue import call, ptr, require

LATTICE_CHUNK = 1 << 20      # lattice points per pnr_lattice_points launch / density() call


def _triple(v, cast):
    if torch.is_tensor(v):
        v = v.detach().cpu().tolist()
    v = list(np.atleast_1d(v)) if not isinstance(v, (list, tuple)) else list(v)
    if len(v) == 1:
        v = v * 3
    if len(v) != 3:
        raise ValueError("expected a scalar or three values")
    return [cast(x) for x in v]


def lattice_points(bound_min, bound_max, resolution, first, count, device):
    """Points first .. first + count of the lattice (C order, z fastest) as a [count, 3] fp32 device tensor (pnr_lattice_points)."""
    lo, hi, n = _triple(bound_min, float), _triple(bound_max, float), _triple(resolution, int)
    pts = torch.empty(count, 3, dtype=torch.float32, device=device)
    with torch.cuda.device(pts.device):
        call("pnr_lattice_points", (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), (ctypes.c_uint32 * 3)(*n), ctypes.c_uint64(first),
             ctypes.c_uint32(count), ptr(pts))
    return pts


def _fused_lattice_density(model, lo, hi, n, device):
    """pnr_lattice_density: the whole volume in one C-ABI call, for the field renderer._fused_sweep_ok describes."""
    enc = model.encoder
    u = torch.empty(n[0] * n[1] * n[2], dtype=torch.float32, device=device)
    lib = _lib.load()
    chunk = min(LATTICE_CHUNK, (u.numel() + 255) // 256 * 256)
    ws = torch.empty(int(lib.pnr_lattice_density_workspace_bytes(chunk)), dtype=torch.uint8, device=device)
    a = _lib.LatticeDensityArgs()
    for d in range(3):
        a.box_min[d], a.box_max[d], a.n[d] = lo[d], hi[d], n[d]
    a.bound = float(model.bound)
    a.embeddings, a.offsets = enc.embeddings.detach().data_ptr(), enc.offsets.data_ptr()
    a.num_levels, a.S, a.base_resolution, a.gridtype = enc.num_levels, float(math.log2(enc.per_level_scale)), enc.base_resolution, enc.gridtype_id
    a.packed_sigma_net = model._sigma_blob().data_ptr()
    a.workspace, a.workspace_bytes, a.u = ws.data_ptr(), ws.numel(), u.data_ptr()
    with torch.cuda.device(device):
        call("pnr_lattice_density", ctypes.byref(a))
    return u.view(*n)


@torch.no_grad()
def lattice_density(model=None, bound_min=None, bound_max=None, resolution=256, query_func=None, device=None):
    """u[x, y, z] = density at the lattice points, as a device tensor.  The shipped field evaluated by its own density() (_fused_sweep_ok) outside
    autocast: one fused call.  Otherwise query_func(pts) -> sigma, or model.density(pts)['sigma'], on chunks of LATTICE_CHUNK points made on the
    device, the way update_extra_state's generic branch asks a field it has no kernel for.  Nothing is read back."""
    if query_func is None:
        if model is None:
            raise ValueError("lattice_density needs a model or a query_func")
        if bound_min is None:
            bound_min, bound_max = model.aabb_infer[:3], model.aabb_infer[3:]
        sweep_ok = getattr(model, "_fused_sweep_ok", None)
        if sweep_ok is not None and sweep_ok() and not torch.is_autocast_enabled():
            return _fused_lattice_density(model, _triple(bound_min, float), _triple(bound_max, float), _triple(resolution, int),
                                          model.encoder.embeddings.device)
        query_func = lambda pts: model.density(pts)["sigma"]
    if device is None:
        if model is not None:
            device = next(model.parameters()).device
        else:
            device = torch.device("cuda", torch.cuda.current_device())
    n = _triple(resolution, int)
    total = n[0] * n[1] * n[2]
    u = torch.empty(total, dtype=torch.float32, device=device)
    for first in range(0, total, LATTICE_CHUNK):
        count = min(LATTICE_CHUNK, total - first)
        pts = lattice_points(bound_min, bound_max, n, first, count, device)
        u[first:first + count] = query_func(pts).reshape(-1).detach().to(device=device, dtype=torch.float32)
    return u.view(*n)


def extract_fields(bound_min, bound_max, resolution, query_func):
    """The reference's extract_fields (nerf/utils.py:187-202): the density volume as a numpy array."""
    return lattice_density(None, bound_min, bound_max, resolution, query_func=query_func).cpu().numpy()


def marching_cubes(u, threshold):
    """mcubes.marching_cubes(u, threshold): (vertices [nv, 3] fp32 in lattice-index coordinates, triangles [nt, 3] int32).  A device tensor in
    gives device tensors out, a numpy array in gives numpy out.  One read-back of the two counts, then exact-size buffers; an empty surface is
    a valid result."""
    as_numpy = not torch.is_tensor(u)
    if as_numpy:
        u = torch.from_numpy(np.array(u, dtype=np.float32, order="C")).cuda()
    if u.ndim != 3:
        raise ValueError("marching_cubes expects a 3-D volume")
    u = require(u.contiguous() if u.dtype == torch.float32 else u.float().contiguous(), torch.float32, "u")
    nx, ny, nz = (int(v) for v in u.shape)
    need = int(_lib.load().pnr_mesh_workspace_bytes(nx, ny, nz))
    if need == 0:
        raise ValueError(f"marching_cubes: every axis of the volume must have 2 .. 512 points, got {(nx, ny, nz)}")
    dev = u.device
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        dims = (ctypes.c_uint32(nx), ctypes.c_uint32(ny), ctypes.c_uint32(nz))
        thr = ctypes.c_float(float(threshold))
        call("pnr_mesh_count", ptr(u), *dims, thr, ptr(ws), ctypes.c_uint64(need), ptr(counts))
        nv, nt = (int(v) for v in counts.cpu().tolist())
        vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(nt, 3, dtype=torch.int32, device=dev)
        call("pnr_mesh_emit", ptr(u), *dims, thr, ptr(ws), ctypes.c_uint64(need), ptr(vertices) if nv else None, ctypes.c_uint32(nv),
             ptr(triangles) if nt else None, ctypes.c_uint32(nt))
    if as_numpy:
        return vertices.cpu().numpy(), triangles.cpu().numpy()
    return vertices, triangles


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func=None, model=None):
    """The reference's extract_geometry (nerf/utils.py:205-217): numpy vertices in world coordinates (float64, v / (R - 1) * (max - min) + min
    as the reference forms them) and int32 triangles."""
    u = lattice_density(model, bound_min, bound_max, resolution, query_func=query_func)
    vertices, triangles = marching_cubes(u, threshold)
    lo, hi = np.asarray(_triple(bound_min, float), np.float32), np.asarray(_triple(bound_max, float), np.float32)
    n = np.asarray(_triple(resolution, int), np.float64)
    v = vertices.cpu().numpy() / (n - 1.0)[None, :] * (hi - lo)[None, :] + lo[None, :]
    return v, triangles.cpu().numpy()


def _density_gradient_fused(model, points, want):
    """pnr_density_gradient on [n, 3] fp32 device points: one launch, raw weights, no workspace."""
    enc, net = model.encoder, model.sigma_net
    n = points.shape[0]
    dev = points.device
    out = {k: torch.empty((n,) if k == "logit" else (n, 3), dtype=torch.float32, device=dev) for k in want}
    a = _lib.DensityGradientArgs()
    a.points, a.n, a.bound = points.data_ptr(), n, float(model.bound)
    a.embeddings, a.offsets = enc.embeddings.detach().data_ptr(), enc.offsets.data_ptr()
    a.num_levels, a.S, a.base_resolution, a.gridtype = enc.num_levels, float(math.log2(enc.per_level_scale)), enc.base_resolution, enc.gridtype_id
    w0, w1 = net[0].weight.detach().contiguous(), net[1].weight.detach().contiguous()
    a.sigma0, a.sigma1 = w0.data_ptr(), w1.data_ptr()
    for k in want:
        setattr(a, k, out[k].data_ptr())
    with torch.cuda.device(dev):
        call("pnr_density_gradient", ctypes.byref(a))
    return out


def _normal_of(grad):
    """-grad / |grad|, and (0, 0, 0) where |grad| is zero or not finite."""
    length = grad.norm(dim=-1, keepdim=True)
    ok = torch.isfinite(grad).all(dim=-1, keepdim=True) & torch.isfinite(length) & (length > 0)
    return torch.where(ok, -grad / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(grad))


def density_gradient_per_op(model, points):
    """{"sigma" [n], "grad" [n, 3], "normal" [n, 3]} by autograd through model.density(): grad = d log(sigma) / d points.  The formulation for
    any field -- another architecture, a density() replaced on the instance (it is asked, not bypassed) -- and the fp32 yardstick the fused kernel
    is tested against.  A sigma that does not depend on the points gives a zero gradient; sigma = 0 gives a gradient that is not finite and a
    zero normal."""
    with torch.enable_grad():
        x = points.detach().clone().requires_grad_()
        sigma = model.density(x)["sigma"].reshape(-1)
        if sigma.requires_grad:
            grad, = torch.autograd.grad(torch.log(sigma).sum(), x)
        else:
            grad = torch.zeros_like(x)
    sigma, grad = sigma.detach().float(), grad.detach().float()
    return {"sigma": sigma, "grad": grad, "normal": _normal_of(grad)}


def density_gradient(model, points, want=("sigma", "grad", "normal")):
    """Density, the gradient of its logarithm and the outward unit normal -grad / |grad| at [n, 3] world-space points, as device tensors: the keys
    of `want` out of "sigma" [n], "grad" [n, 3], "normal" [n, 3].  The shipped field evaluated by its own density() (_fused_sweep_ok) outside
    autocast: one pnr_density_gradient launch.  Anything else: density_gradient_per_op."""
    want = tuple(want)
    if not want or any(k not in ("sigma", "grad", "normal") for k in want):
        raise ValueError('density_gradient: want is a non-empty subset of ("sigma", "grad", "normal")')
    sweep_ok = getattr(model, "_fused_sweep_ok", None)
    if sweep_ok is not None and sweep_ok() and points.is_cuda and not torch.is_autocast_enabled():
        pts = points.detach().reshape(-1, 3)
        pts = require(pts.contiguous() if pts.dtype == torch.float32 else pts.float().contiguous(), torch.float32, "points")
        if pts.shape[0] == 0:
            return {k: torch.empty((0,) if k == "sigma" else (0, 3), dtype=torch.float32, device=pts.device) for k in want}
        out = _density_gradient_fused(model, pts, tuple("logit" if k == "sigma" else k for k in want))
        if "logit" in out:
            out["sigma"] = torch.exp(out.pop("logit"))
        return out
    full = density_gradient_per_op(model, points.reshape(-1, 3))
    return {k: full[k] for k in want}


@torch.no_grad()
def vertex_attributes(model, world_points, chunk=None):
    """What a recolourable mesh carries per vertex, as device tensors, for [nv, 3] fp32 world-space points in chunks of `chunk` (LATTICE_CHUNK):
    normal from density_gradient, then the model's own forward at the view direction d = -normal ((0, 0, 1) where the normal is zero).
      NeRF model:        normal, rgb
      PaletteNeRF model: normal, diffuse, view_dep, omega [nv, nb], radiance [nv] (softplus of the raw value), offsets [nv, nb, 3],
                         base_rgb = sum_b omega_b radiance (clamp(P_b, 0, 1) + offsets_weight offsets_b), rgb = base_rgb + view_dep_weight view_dep
                         (the renderer's composite without edit or stylizer), and clip_feat with a clip head."""
    chunk = int(chunk or LATTICE_CHUNK)
    pts = world_points.detach().reshape(-1, 3).float().contiguous()
    palette = hasattr(model, "basis_color")
    if pts.shape[0] == 0:      # an empty surface: the same keys, no rows, no launch
        def none(*shape):
            return torch.empty((0,) + shape, dtype=torch.float32, device=pts.device)
        if not palette:
            return {"normal": none(3), "rgb": none(3)}
        nb = int(model.num_basis)
        out = {"normal": none(3), "diffuse": none(3), "view_dep": none(3), "omega": none(nb), "radiance": none(), "offsets": none(nb, 3),
               "base_rgb": none(3), "rgb": none(3)}
        if getattr(model.opt, "pred_clip", False):
            out["clip_feat"] = none(int(model.opt.clip_dim))
        return out
    parts = []
    for first in range(0, pts.shape[0], chunk):
        x = pts[first:first + chunk]
        normal = density_gradient(model, x, want=("normal",))["normal"]
        up = torch.zeros_like(normal)
        up[:, 2] = 1
        d = torch.where((normal == 0).all(dim=-1, keepdim=True), up, -normal).contiguous()
        if not palette:
            _, rgb = model(x, d)
            parts.append({"normal": normal, "rgb": rgb.float().reshape(-1, 3)})
            continue
        nb = int(model.num_basis)
        M = x.shape[0]
        _, clip_feat, omega, offsets_radiance, view_dep, diffuse = model(x, d, frozen_density=True)
        omega = omega.float().reshape(M, nb)
        offsets_radiance = offsets_radiance.float().reshape(M, 3 * nb + 1)
        offsets, radiance = offsets_radiance[:, :-1].reshape(M, nb, 3), torch.nn.functional.softplus(offsets_radiance[:, -1])
        view_dep, diffuse = view_dep.float().reshape(M, 3), diffuse.float().reshape(M, 3)
        basis = model.basis_color.detach().float().clamp(0, 1)[None, :, :]
        final = radiance[:, None, None] * (basis + float(getattr(model, "offsets_weight", 1)) * offsets)
        base_rgb = (omega[:, :, None] * final).sum(dim=-2)
        part = {"normal": normal, "diffuse": diffuse, "view_dep": view_dep, "omega": omega, "radiance": radiance, "offsets": offsets.contiguous(),
                "base_rgb": base_rgb, "rgb": base_rgb + float(getattr(model, "view_dep_weight", 1)) * view_dep}
        if getattr(model.opt, "pred_clip", False):
            part["clip_feat"] = clip_feat.float().reshape(M, -1)
        parts.append(part)
    return {k: torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in parts[0]}


def vertex_records(vertices, bound_min, bound_max, resolution, normal=None, rgb=None, extra=None, linear_to_srgb=False, want_records=True):
    """pnr_mesh_vertex_records: (world [nv, 3] fp32, records [nv, record_bytes] uint8 or None) on the device from marching_cubes' lattice-index
    vertices.  world is extract_geometry's float64 vertex rounded once to fp32; a record is x y z | normal | rgba | extra (little endian)."""
    lo, hi, n = _triple(bound_min, float), _triple(bound_max, float), _triple(resolution, int)
    v = require(vertices.contiguous(), torch.float32, "vertices")
    nv, dev = v.shape[0], v.device

    def f32(t, name, cols):
        if t is None:
            return None
        t = require(t.detach().contiguous(), torch.float32, name)
        if t.shape[0] != nv or (cols is not None and tuple(t.shape[1:]) != (cols,)):
            raise ValueError(f"vertex_records: {name} does not match the vertices")
        return t

    normal, rgb, extra = f32(normal, "normal", 3), f32(rgb, "rgb", 3), f32(extra, "extra", None)
    channels = 0 if extra is None else int(extra.shape[1])
    world = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    records = None
    if want_records:
        size = int(_lib.load().pnr_mesh_vertex_record_bytes(int(normal is not None), int(rgb is not None), channels))
        records = torch.empty(nv, size, dtype=torch.uint8, device=dev)
    if nv == 0:      # an empty surface: nothing to launch (and an empty tensor has no address to pass)
        return world, records
    a = _lib.VertexRecordsArgs()
    a.vertices, a.nv = v.data_ptr(), nv
    for d in range(3):
        a.box_min[d], a.box_max[d], a.n[d] = lo[d], hi[d], n[d]
    a.normal, a.rgb, a.linear_to_srgb = ptr(normal), ptr(rgb), int(bool(linear_to_srgb))
    a.extra, a.extra_channels, a.extra_stride = (ptr(extra) if channels else None), channels, channels
    a.world, a.records = world.data_ptr(), ptr(records)
    with torch.cuda.device(dev):
        call("pnr_mesh_vertex_records", ctypes.byref(a))
    return world, records


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1", "int8": "i1",
              "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}
XYZ_PROPERTIES = (("float", "x"), ("float", "y"), ("float", "z"))
NORMAL_PROPERTIES = (("float", "nx"), ("float", "ny"), ("float", "nz"))
RGBA_PROPERTIES = (("uchar", "red"), ("uchar", "green"), ("uchar", "blue"), ("uchar", "alpha"))


def write_ply(path, vertices, triangles, records=None, properties=None, comments=()):
    """Binary little-endian PLY: float32 x y z, faces as (uchar count, int indices) -- the layout trimesh exports.
    records [nv, record_bytes] uint8 with properties [(type, name), ...]: the vertex block is these bytes as they are (pnr_mesh_vertex_records':
    x y z first) and `vertices` is not read; comments become `comment` lines behind the format line.  Without them: today's bytes."""
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    if records is None:
        if properties is not None:
            raise ValueError("write_ply: properties describe records")
        v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
        nv, block, properties = len(v), v.tobytes(), XYZ_PROPERTIES
    else:
        properties = tuple((str(ty), str(name)) for ty, name in (properties or ()))
        size = sum(np.dtype(_PLY_TYPES[ty]).itemsize for ty, _ in properties)
        r = np.ascontiguousarray(records, dtype=np.uint8)
        if tuple(n for _, n in properties[:3]) != ("x", "y", "z") or r.ndim != 2 or (r.shape[1] != size and len(r)):
            raise ValueError("write_ply: records are [nv, record_bytes] rows whose properties begin with x y z and add up to record_bytes")
        nv, block = len(r), r.tobytes()
    for c in comments:
        if "\n" in c:
            raise ValueError("write_ply: a comment is one line")
    header = ("ply\nformat binary_little_endian 1.0\n" + "".join(f"comment {c}\n" for c in comments)
              + f"element vertex {nv}\n" + "".join(f"property {ty} {name}\n" for ty, name in properties)
              + f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(block)
        f.write(faces.tobytes())


def _ply_header(data):
    """(offset of the vertex block, nv, nt, vertex dtype, comments) of a file write_ply wrote."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply reads the binary little-endian files write_ply writes")
    nv = nt = None
    element, fields, comments = None, [], []
    for line in lines[2:]:
        word = line.split()
        if not word:
            continue
        if word[0] == "comment":
            comments.append(line[len("comment "):])
        elif word[0] == "element":
            element = word[1]
            if element == "vertex":
                nv = int(word[2])
            elif element == "face":
                nt = int(word[2])
        elif word[0] == "property" and element == "vertex":
            if word[1] == "list" or word[1] not in _PLY_TYPES:
                raise ValueError("read_ply: scalar vertex properties only")
            fields.append((word[2], _PLY_TYPES[word[1]]))
    return end, nv, nt, np.dtype(fields), comments


def read_ply(path):
    """What write_ply wrote: (vertices [nv, 3] float32, triangles [nt, 3] int32); further vertex properties are skipped."""
    with open(path, "rb") as f:
        data = f.read()
    end, nv, nt, vdtype, _ = _ply_header(data)
    block = np.frombuffer(data, dtype=vdtype, count=nv, offset=end)
    v = np.stack([block["x"], block["y"], block["z"]], axis=1).astype(np.float32).reshape(nv, 3)
    faces = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nt, offset=end + nv * vdtype.itemsize)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("read_ply: only triangles")
    return v, faces["i"].astype(np.int32).reshape(nt, 3)


def read_ply_attributes(path):
    """({vertex property name: array [nv], ..., "triangles": [nt, 3] int32}, comment lines) of a file write_ply wrote."""
    with open(path, "rb") as f:
        data = f.read()
    end, nv, nt, vdtype, comments = _ply_header(data)
    block = np.frombuffer(data, dtype=vdtype, count=nv, offset=end)
    out = {name: np.ascontiguousarray(block[name]) for name in vdtype.names}
    faces = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nt, offset=end + nv * vdtype.itemsize)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("read_ply_attributes: only triangles")
    out["triangles"] = faces["i"].astype(np.int32).reshape(nt, 3)
    return out, comments


def palette_properties(num_basis):
    """The float properties behind rgba in an attributes="palette" file, in record order: radiance, omega_b, offset_b_{r,g,b}."""
    names = ["radiance"] + [f"omega_{b}" for b in range(num_basis)] + [f"offset_{b}_{c}" for b in range(num_basis) for c in "rgb"]
    return tuple(("float", n) for n in names)


def save_mesh(model, save_path, resolution=256, threshold=10, attributes=None, linear_to_srgb=False):
    """Trainer.save_mesh (nerf/utils.py:633-653): density over aabb_infer -> marching cubes -> .ply.
    attributes: None -- bare geometry, the reference's file; "color" -- normals and rgba per vertex (rgb of a NeRF model, base_rgb of a PaletteNeRF
    model; linear_to_srgb as in image_to_uint8); "palette" (PaletteNeRF) -- additionally the float properties of palette_properties() and one
    `comment palette <b> <r> <g> <b>` line per basis, the clamped palette: a recolourable asset.  The vertex block is formed on the device
    (vertex_attributes, vertex_records).  Returns (vertices, triangles), and the attribute dict as a third value when attributes were asked."""
    if attributes not in (None, "color", "palette"):
        raise ValueError('save_mesh: attributes is None, "color" or "palette"')
    palette = hasattr(model, "basis_color")
    if attributes == "palette" and not palette:
        raise ValueError('save_mesh: attributes="palette" needs a PaletteNeRF model')
    d = os.path.dirname(save_path)
    if d:
        os.makedirs(d, exist_ok=True)
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
    if attributes is None:
        vertices, triangles = extract_geometry(lo, hi, resolution, threshold, model=model)
        write_ply(save_path, vertices, triangles)
        return vertices, triangles
    u = lattice_density(model, lo, hi, resolution)
    vertices, triangles = marching_cubes(u, threshold)
    del u
    world, _ = vertex_records(vertices, lo, hi, resolution, want_records=False)
    attrs = vertex_attributes(model, world)
    nv = vertices.shape[0]
    properties, comments, extra = XYZ_PROPERTIES + NORMAL_PROPERTIES + RGBA_PROPERTIES, [], None
    if attributes == "palette":
        nb = int(model.num_basis)
        extra = torch.cat([attrs["radiance"].reshape(nv, 1), attrs["omega"].reshape(nv, nb), attrs["offsets"].reshape(nv, 3 * nb)], dim=1).contiguous()
        properties = properties + palette_properties(nb)
        basis = model.basis_color.detach().float().clamp(0, 1).cpu().numpy()
        comments = [f"palette {b} {float(c[0]):.9g} {float(c[1]):.9g} {float(c[2]):.9g}" for b, c in enumerate(basis)]
    _, records = vertex_records(vertices, lo, hi, resolution, normal=attrs["normal"], rgb=attrs["base_rgb" if palette else "rgb"], extra=extra,
                                linear_to_srgb=linear_to_srgb)
    triangles = triangles.cpu().numpy()
    write_ply(save_path, None, triangles, records=records.cpu().numpy(), properties=properties, comments=comments)
    lo32, hi32 = np.asarray(_triple(lo, float), np.float32), np.asarray(_triple(hi, float), np.float32)
    n = np.asarray(_triple(resolution, int), np.float64)
    v = vertices.cpu().numpy() / (n - 1.0)[None, :] * (hi32 - lo32)[None, :] + lo32[None, :]
    return v, triangles, attrs
