"""Mesh export: the tail of the reference's Trainer.save_mesh (nerf/utils.py:187-217, :633-653) on the device.

The reference queries density() on a resolution^3 lattice in blocks built with linspace / meshgrid / cat, reads every block back, runs PyMCubes
on the CPU and lets trimesh write a .ply.  Here the shipped field fills a device volume in one call (pnr_lattice_density: the occupancy sweep's
lookup and sigma_net kernels on lattice points), any other field is handed the points in chunks (pnr_lattice_points) and asked through its own
density(), marching cubes runs over the volume on the device (csrc/mesh.hip: count, one scan, emit) and the host reads back two counts and the
exact-size result.  The vertex and triangle order is fixed (include/pnr.h), so the output is reproducible bit for bit.

Triangles are counter-clockwise seen from the low-density side (normals point out of the dense region).
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


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: float32 x y z, faces as (uchar count, int indices) -- the layout trimesh exports."""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """What write_ply wrote: (vertices [nv, 3] float32, triangles [nt, 3] int32)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply reads the binary little-endian files write_ply writes")
    nv = nt = None
    for line in lines:
        if line.startswith("element vertex"):
            nv = int(line.split()[2])
        elif line.startswith("element face"):
            nt = int(line.split()[2])
    v = np.frombuffer(data, dtype="<f4", count=nv * 3, offset=end).reshape(nv, 3).astype(np.float32)
    faces = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nt, offset=end + nv * 12)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("read_ply: only triangles")
    return v, faces["i"].astype(np.int32).reshape(nt, 3)


def save_mesh(model, save_path, resolution=256, threshold=10):
    """Trainer.save_mesh (nerf/utils.py:633-653): density over aabb_infer -> marching cubes -> .ply."""
    d = os.path.dirname(save_path)
    if d:
        os.makedirs(d, exist_ok=True)
    vertices, triangles = extract_geometry(model.aabb_infer[:3], model.aabb_infer[3:], resolution, threshold, model=model)
    write_ply(save_path, vertices, triangles)
    return vertices, triangles
