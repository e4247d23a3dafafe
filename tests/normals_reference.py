"""Float64 statement of the coloured mesh export's two device stages (include/pnr.h, "coloured mesh export").  TEST HELPER, not a test; numpy and
torch float64 on the CPU, no GPU.

Density gradient: logit = sigma_net(encoder((p + bound) / (2 bound)))[0] and d logit / d p of the shipped field.  The encoder's value and its per-level
derivative are tests/grid_reference.GridReference's forward and dy_dx -- float64 behind the fp32 cell position the kernels share -- and sigma_net is
two float64 matrix products with the ReLU's derivative z > 0.  What is shared with the code under test is the input alone: the fp32 unit-cube
coordinate (p + bound) / (2 bound), two fp32 roundings as grid_xside.hpp:unit_cube_of forms it.

Vertex records: the bytes of pnr_mesh_vertex_records, stated in numpy from the contract."""
import numpy as np
import torch

from tests.grid_reference import GridReference


def unit_cube(points, bound):
    """(p + bound) / (2 bound) in fp32: a sum and a quotient, each rounded (for 2 bound a power of two the kernels' exact reciprocal gives the same bits)"""
    p = np.asarray(points, np.float32)
    return ((p + np.float32(bound)).astype(np.float32) / np.float32(2.0 * bound)).astype(np.float32)


class DensityField:
    """The shipped density field as numpy arrays: table [rows, 2], offsets [17], per_level_scale, base_resolution, gridtype, sigma0 [64, 32], sigma1 [16, 64]."""

    def __init__(self, table, offsets, per_level_scale, base_resolution, gridtype, sigma0, sigma1, bound):
        self.table = np.asarray(table, np.float32)
        self.offsets = np.asarray(offsets).astype(np.int64)
        self.per_level_scale, self.base_resolution, self.gridtype, self.bound = float(per_level_scale), int(base_resolution), int(gridtype), float(bound)
        self.sigma0, self.sigma1 = np.asarray(sigma0, np.float64), np.asarray(sigma1, np.float64)
        assert self.table.shape[1] == 2 and len(self.offsets) == 17 and self.sigma0.shape == (64, 32) and self.sigma1.shape[1] == 64

    @classmethod
    def of_model(cls, model):
        enc = model.encoder
        return cls(enc.embeddings.detach().cpu().numpy(), enc.offsets.cpu().numpy(), enc.per_level_scale, enc.base_resolution, enc.gridtype_id,
                   model.sigma_net[0].weight.detach().cpu().numpy(), model.sigma_net[1].weight.detach().cpu().numpy(), model.bound)

    def geometry(self, points):
        return GridReference(unit_cube(points, self.bound), self.offsets, self.per_level_scale, self.base_resolution, self.gridtype, False)

    def evaluate(self, points, geometry=None):
        """points [n, 3] fp32 world space -> dict of float64 arrays:
        logit [n], grad [n, 3] (d logit / d p, world), enc [n, 32], z [n, 64] hidden pre-activations, inside [n] bool, normal [n, 3] (-grad / |grad|, 0 where
        grad is 0)."""
        ref = geometry or self.geometry(points)
        enc, _ = ref.forward(self.table)                      # [n, 16, 2]
        dy, _ = ref.dy_dx(self.table)                         # [n, 16, 3, 2], d enc / d x in unit-cube coordinates
        enc = enc.reshape(ref.B, 32)                          # column 2 l + c
        z = enc @ self.sigma0.T
        w1 = self.sigma1[0]
        logit = np.maximum(z, 0.0) @ w1
        a = (z > 0) * w1[None, :]                             # d logit / d z
        c = (a @ self.sigma0).reshape(ref.B, 16, 1, 2)        # d logit / d enc
        grad = (c * dy).sum(axis=(1, 3)) / (2.0 * self.bound)
        length = np.linalg.norm(grad, axis=1, keepdims=True)
        normal = np.where(length > 0, -grad / np.where(length > 0, length, 1.0), 0.0)
        return {"logit": logit, "grad": grad, "enc": enc, "z": z, "inside": ref.inr.copy(), "normal": normal}


def set_positions(ref, x64):
    """Replace a GridReference's in-cell fractions by those of float64 unit-cube positions x64 [n, 3] IN THE SAME CELLS (asserted): the statement as
    a function of a real-valued position, for difference quotients.  The rows stay those of the fp32 points the reference was built on."""
    x64 = np.asarray(x64, np.float64)
    for l in range(ref.L):
        pos = x64 * ref.scale[l] + 0.5
        pg = np.floor(pos)
        fr = pos - pg
        assert np.array_equal(pg, np.floor(ref._base_pos(l))), "a moved point left its cell"
        ref.f[l, :, 0], ref.f[l, :, 1] = (1.0 - fr).T, fr.T
    return ref


class RealPositionGeometry(GridReference):
    """GridReference that remembers the fp32 points it was built on, so that set_positions can assert the cells."""

    def __init__(self, x, *args):
        super().__init__(x, *args)
        self._x = np.asarray(x, np.float32).astype(np.float64)

    def _base_pos(self, l):
        return (self._x * self.scale[l] + 0.5).astype(np.float32).astype(np.float64)


def srgb_bytes(rgb, linear_to_srgb):
    """[nv, 3] fp32 -> uint8: (uint8)(int)(s(clamp(c, 0, 1)) * 255.0f) in fp32, NaN as 0."""
    x = np.asarray(rgb, np.float32)
    x = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    if linear_to_srgb:
        curve = (np.float32(1.055) * np.power(x, np.float32(0.41666)).astype(np.float32)).astype(np.float32) - np.float32(0.055)
        x = np.where(x < np.float32(0.0031308), (np.float32(12.92) * x).astype(np.float32), curve.astype(np.float32)).astype(np.float32)
    return (x * np.float32(255.0)).astype(np.float32).astype(np.int32).astype(np.uint8)


def world_vertices(vertices, lo, hi, n):
    """extract_geometry's float64 expression: v / (n - 1) * (hi - lo) + lo with hi - lo subtracted in fp32."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    n = np.asarray(n, np.float64)
    return np.asarray(vertices, np.float32) / (n - 1.0)[None, :] * (hi - lo)[None, :] + lo[None, :]


def vertex_records(vertices, lo, hi, n, normal=None, rgb=None, linear_to_srgb=False, extra=None):
    """(world [nv, 3] fp32, records [nv, record_bytes] uint8): x y z | nx ny nz | red green blue alpha | extra..., little endian."""
    world = world_vertices(vertices, lo, hi, n).astype("<f4")
    nv = len(world)
    cols = [np.ascontiguousarray(world).view(np.uint8).reshape(nv, 12)]
    if normal is not None:
        cols.append(np.ascontiguousarray(normal, dtype="<f4").view(np.uint8).reshape(nv, 12))
    if rgb is not None:
        cols.append(np.concatenate([srgb_bytes(rgb, linear_to_srgb).reshape(nv, 3), np.full((nv, 1), 255, np.uint8)], axis=1))
    if extra is not None and np.asarray(extra).shape[1]:
        e = np.ascontiguousarray(extra, dtype="<f4")
        cols.append(e.view(np.uint8).reshape(nv, 4 * e.shape[1]))
    return world.astype(np.float32), np.concatenate(cols, axis=1)


def ambiguous_rows(enc, sigma0, margin=2e-5):
    """tests/float64_blocks.mlp_ambiguous on the hidden layer: rows with a pre-activation within `margin` of the ReLU's kink in float64."""
    from tests.float64_blocks import mlp_ambiguous
    w = [torch.from_numpy(np.asarray(sigma0, np.float64)), torch.zeros(1, 64, dtype=torch.float64)]
    return mlp_ambiguous(torch.from_numpy(np.asarray(enc, np.float64)), w, torch.relu, "cpu", margin=margin).numpy()
