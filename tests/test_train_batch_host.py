"""Training batches, the parts that need no device: the float64 statement of the weight guide against grid_sample in double, uint8 storage,
TrainSet's refusals, draw_indices against the index logic get_rays had, the ctypes mirror against the header, the entries' validation."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from palettenerf_amd import _lib, rays, trainset
from tests import train_batch_reference as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def guide_colours(S, n_random, seed):
    """The four kinds of colour the guide is checked at: exactly 0, exactly 1, bin nodes i / (S - 1), random."""
    g = np.random.default_rng(seed)
    nodes = g.integers(0, S, size=(64, 3)) / (S - 1)
    mixed = np.stack([np.array([0.0, 1.0, 0.5]), np.array([1.0, 0.0, 1.0]), np.array([0.25, 1.0, 0.0])])
    return np.concatenate([np.zeros((1, 3)), np.ones((1, 3)), mixed, nodes, g.random((n_random, 3))])


@pytest.mark.parametrize("nb,S", [(4, (32, 32, 32)), (5, (8, 8, 8)), (8, (5, 7, 9))])
def test_float64_guide_statement_is_grid_sample_in_double(nb, S):
    g = np.random.default_rng(nb)
    hist = g.random((nb, *S))
    rgb = guide_colours(min(S), 500, 1)
    if len(set(S)) > 1:       # bin nodes of an uneven table, per axis
        rgb[5:69] = np.stack([g.integers(0, s, size=64) / (s - 1) for s in S], -1)
    mine = ref.lut_f64(rgb, hist)
    theirs = ref.lut_torch(torch.from_numpy(rgb), torch.from_numpy(hist)[None]).numpy()
    # grid_sample forms its coordinate as ((2c - 1) + 1) / 2 (S - 1): <= 4 eps (S - 1) from c (S - 1); the table's values lie in [0, 1], so a
    # coordinate error d moves the result by <= d per axis; plus the 8-term sum's own rounding
    bound = (12 * (max(S) - 1) + 8) * np.finfo(np.float64).eps
    err = np.abs(mine - theirs).max()
    print(f"nb={nb} S={S}: float64 statement vs grid_sample(double) {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    assert np.array_equal(mine[0], hist[:, 0, 0, 0]) and np.array_equal(mine[1], hist[:, -1, -1, -1])      # exactly 0 and exactly 1: the corner itself
    node = np.rint(rgb[5:69] * (np.array(S) - 1)).astype(int)
    assert np.abs(mine[5:69] - hist[:, node[:, 0], node[:, 1], node[:, 2]].T).max() <= 64 * np.finfo(np.float64).eps   # r is the slowest axis
    planes = hist / hist.sum(0, keepdims=True)
    assert np.abs(ref.lut_f64(rgb, planes).sum(-1) - 1).max() <= 1e-14


def test_uint8_storage_is_the_loaders_division():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 8, 8, 4)
    want = u8.astype(np.float32) / 255
    assert np.array_equal(ref.decode(u8), want)
    assert np.array_equal((torch.from_numpy(u8).float() / 255).numpy(), want)
    ts = trainset.TrainSet(want, np.eye(4, dtype=np.float32)[None], (10.0, 10.0, 4.0, 4.0), 8, 8, 16, storage="uint8", device="cpu")
    assert ts.images.dtype == torch.uint8 and np.array_equal(ts.images.numpy(), u8)          # a float stack from 8-bit files comes back exactly
    ts = trainset.TrainSet(u8, np.eye(4, dtype=np.float32)[None], (10.0, 10.0, 4.0, 4.0), 8, 8, 16, storage="uint8", device="cpu")
    assert np.array_equal(ts.images.numpy(), u8)
    half = trainset.TrainSet(u8, np.eye(4, dtype=np.float32)[None], (10.0, 10.0, 4.0, 4.0), 8, 8, 16, storage="fp16", device="cpu")
    assert half.images.dtype == torch.float16 and np.array_equal(half.images.numpy(), want.astype(np.float16))
    assert ts.num_rays == 16 and len(ts) == 1 and ts.error_map is None
    with pytest.raises(RuntimeError, match="CUDA"):
        ts.batch(0)                                    # no CPU path exists


def test_trainset_refuses_what_it_cannot_hold():
    pose = np.eye(4, dtype=np.float32)[None].repeat(2, 0)
    intr = (10.0, 10.0, 4.0, 3.0)
    img = np.zeros((2, 6, 8, 4), np.float32)
    mk = lambda **kw: trainset.TrainSet(**{**dict(images=img, poses=pose, intrinsics=intr, H=6, W=8, num_rays=16, device="cpu"), **kw})   # noqa: E731
    mk()
    with pytest.raises(ValueError, match=r"\[V,H,W,C\]"):
        mk(images=img[0])
    with pytest.raises(ValueError, match="3 or 4 channels"):
        mk(images=img[..., :2])
    with pytest.raises(ValueError, match="H x W"):
        mk(H=8, W=6)
    with pytest.raises(ValueError, match="poses"):
        mk(poses=pose[:1])
    with pytest.raises(ValueError, match="poses"):
        mk(poses=pose[:, :3])
    with pytest.raises(ValueError, match="must divide"):
        mk(patch_size=3)
    mk(patch_size=4)
    with pytest.raises(ValueError, match="even"):
        mk(random_size=5, num_rays=15)
    with pytest.raises(ValueError, match="feat_images"):
        mk(feat_images=np.zeros((2, 6, 7, 16), np.float32))
    with pytest.raises(ValueError, match="storage"):
        mk(storage="bf16")
    with pytest.raises(ValueError, match="color_space"):
        mk(color_space="hsv")
    with pytest.raises(ValueError, match="positive"):
        mk(num_rays=0)
    ts = mk(error_map=True, num_rays=1000)
    assert ts.num_rays == 48 and ts.error_map.shape == (2, 128 * 128) and float(ts.error_map.min()) == 1.0     # capped at H W, as get_rays does
    with pytest.raises(IndexError):
        ts._view_index(2)
    with pytest.raises(IndexError):
        ts._view_index([0, -1])


def legacy_indices(H, W, N, error_map, patch_size, random_size, B, device):
    """The index selection as rays.get_rays had it inline before draw_indices existed."""
    if patch_size > 1:
        n_patches = N // (patch_size * patch_size)
        top = torch.randint(0, H - patch_size, size=[n_patches], device=device)
        left = torch.randint(0, W - patch_size, size=[n_patches], device=device)
        dy, dx = torch.meshgrid(torch.arange(patch_size, device=device), torch.arange(patch_size, device=device), indexing="ij")
        return ((top[:, None] + dy.reshape(1, -1)) * W + left[:, None] + dx.reshape(1, -1)).reshape(-1).expand(B, -1), None
    if random_size > 0:
        half = N // 2
        y0 = torch.randint(0, H, size=[half], device=device)
        x0 = torch.randint(0, W, size=[half], device=device)
        jy = torch.randint(-random_size, random_size, size=[half], device=device)
        jx = torch.randint(-random_size, random_size, size=[half], device=device)
        return torch.cat([y0 * W + x0, (y0 + jy).clamp(0, H - 1) * W + (x0 + jx).clamp(0, W - 1)], dim=0).expand(B, -1), None
    if error_map is None:
        return torch.randint(0, H * W, size=[N], device=device).expand(B, N), None
    coarse = torch.multinomial(error_map.to(device), N, replacement=False)
    cy, cx = coarse // 128, coarse % 128
    sy, sx = H / 128, W / 128
    yy = (cy * sy + torch.rand(B, N, device=device) * sy).long().clamp(max=H - 1)
    xx = (cx * sx + torch.rand(B, N, device=device) * sx).long().clamp(max=W - 1)
    return yy * W + xx, coarse


MODES = {"plain": {}, "patch": dict(patch_size=4), "pairs": dict(random_size=5), "error_map": dict(error_map=True)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("B", [1, 2])
def test_draw_indices_is_get_rays_index_logic_under_one_seed(monkeypatch, mode, B):
    H, W, N = 37, 53, 64
    kw = dict(MODES[mode])
    emap = torch.rand(B, 128 * 128, generator=torch.Generator().manual_seed(5)) if kw.pop("error_map", False) else None
    cpu = torch.device("cpu")
    torch.manual_seed(11)
    want, want_coarse = legacy_indices(H, W, N, emap, kw.get("patch_size", 1), kw.get("random_size", 0), B, cpu)
    after = torch.rand(3)
    torch.manual_seed(11)
    got, got_coarse = rays.draw_indices(H, W, N, emap, kw.get("patch_size", 1), kw.get("random_size", 0), B, cpu)
    assert torch.equal(torch.rand(3), after)                       # the generator stands where it stood: the same number of draws
    assert got.shape == (B, N) and got.dtype == torch.int64 and torch.equal(got, want)
    assert (got_coarse is None) == (want_coarse is None) and (want_coarse is None or torch.equal(got_coarse, want_coarse))
    assert int(got.min()) >= 0 and int(got.max()) < H * W
    # and get_rays itself draws through it (the ray launch stubbed out: no device here)
    monkeypatch.setattr(rays, "rays_from_indices", lambda poses, intr, H, W, inds=None: (torch.zeros(B, N, 3), torch.zeros(B, N, 3)))
    torch.manual_seed(11)
    out = rays.get_rays(torch.eye(4)[None].repeat(B, 1, 1), (50.0, 50.0, W / 2, H / 2), H, W, N, emap, **kw)
    assert torch.equal(out["inds"], want) and ("inds_coarse" in out) == (want_coarse is not None)
    assert list(out)[-3:] == ["inds", "rays_o", "rays_d"]


def header_struct(cname):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnr.h")).read(), flags=re.S)
    body = re.search(r"typedef struct(?: \w+)? \{([^}]*)\} " + cname + ";", hdr).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.sub(r"\[[^\]]*\]", "", part).replace("*", " ").split()[-1] for part in decl.split(",")]
    return names


def test_train_batch_struct_mirror_follows_the_header(tmp_path):
    names = [f[0] for f in _lib.TrainBatchArgs._fields_]
    assert names == header_struct("pnr_train_batch_args")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(pnr_train_batch_args));']
    lines += [f'  printf("{n} %zu\\n", offsetof(pnr_train_batch_args, {n}));' for n in names] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.TrainBatchArgs)
    for n in names:
        assert int(got[n]) == getattr(_lib.TrainBatchArgs, n).offset, n
    assert (_lib.IMAGE_FP32, _lib.IMAGE_FP16, _lib.IMAGE_UINT8) == (0, 1, 2) and _lib.load().pnr_abi_version() == 10
    assert _lib.SIGNATURES["pnr_train_batch"] == [ctypes.c_void_p] * 2 and len(_lib.SIGNATURES["pnr_error_map_update"]) == 8


def test_train_batch_entries_validate_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.pnr_train_batch(None, None) == -1
    a = _lib.TrainBatchArgs()
    assert lib.pnr_train_batch(ctypes.byref(a), None) == 0                    # no rays: a no-op
    a.B, a.N = 1, 16
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # no indices, no stack
    a.view_index = a.inds = p
    a.V, a.H, a.W = 3, 6, 8
    assert lib.pnr_train_batch(ctypes.byref(a), None) == 0                    # nothing asked for
    a.rays_o = p
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # rays_o without rays_d
    a.rays_d = p
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # no poses, fx = 0
    a.rays_o = a.rays_d = None
    a.gt_rgb = p
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # no images
    a.images, a.C = p, 5
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # C
    a.C, a.image_format = 4, 3
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -2                   # format
    a.image_format, a.bg_mode = _lib.IMAGE_UINT8, 3
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # bg_mode
    a.bg_mode = 2
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # ... without its array
    a.bg_mode, a.gt_weights = 0, p
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # no table
    a.hist_weights, a.Sr, a.Sg, a.Sb, a.num_basis = p, 8, 8, 8, 11
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -2                   # more than PNR_MAX_BASIS planes
    a.num_basis, a.Sb = 4, 0
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1
    a.Sb, a.gt_weights, a.gt_clip = 8, None, p
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -1                   # no feature stack
    a.feat_images, a.D, a.feat_format = p, 16, _lib.IMAGE_UINT8
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -2
    a.H = a.W = 1 << 16
    assert lib.pnr_train_batch(ctypes.byref(a), None) == -2                   # pixel ids are 32-bit in the ray arithmetic
    u32 = ctypes.c_uint32
    assert lib.pnr_error_map_update(None, u32(16384), None, None, None, u32(0), u32(8), None) == 0
    assert lib.pnr_error_map_update(None, u32(16384), p, p, p, u32(1), u32(8), None) == -1
    assert lib.pnr_error_map_update(p, u32(0), p, p, p, u32(1), u32(8), None) == -1
