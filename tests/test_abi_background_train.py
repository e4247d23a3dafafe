"""The training entries of the background model on the host: pnr_background_train_forward / pnr_background_backward with their argument struct and
pnr_train_loss_backward_bg (no GPU needed: every check below returns before a launch).  They are additive: the ABI version stays 10 and the
structs of ABI 10 keep their layouts."""
import ctypes
import os
import subprocess

import pytest
import torch

from oracle.torch_encoders import TorchSHEncoder
from palettenerf_amd import _lib, fused, network

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, UNSUPPORTED, ALIGNMENT = -1, -2, -4
FWD_PTRS = ("rays_o", "rays_d", "embeddings", "offsets", "w0", "w1", "out", "coords_out")
BWD_PTRS = ("rays_d", "coords_in", "embeddings", "offsets", "w0", "w1", "grad_rgb", "grad_w0", "grad_w1", "workspace")


def supported(n=0, ptrs=()):
    a = _lib.BackgroundTrainArgs()
    a.num_levels, a.level_dim, a.sh_degree, a.num_layers, a.hidden_dim = 4, 2, 4, 2, 64
    a.N, a.table_rows = n, 64
    for name in ptrs:
        setattr(a, name, 256)
    a.workspace_bytes = 1 << 30
    return a


def c_layout(tmp_path, cname, mirror):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pnr.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, *_ in mirror._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / f"{cname}.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / cname
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())


def test_abi_version_stays_10_and_the_new_entry_points_exist():
    lib = _lib.load()
    assert lib.pnr_abi_version() == 10
    p = ctypes.c_void_p
    assert _lib.SIGNATURES["pnr_background_train_forward"] == [p, p]
    assert _lib.SIGNATURES["pnr_background_backward"] == [p, p]
    assert _lib.SIGNATURES["pnr_background_backward_workspace_bytes"] == [ctypes.c_uint32]
    assert _lib.SIGNATURES["pnr_train_loss_backward_bg"] == [p, p, p]
    with open(os.path.join(ROOT, "include", "pnr.h")) as f:
        header = " ".join(f.read().split())
    for decl in ("int pnr_background_train_forward(const pnr_background_train_args* args, pnr_stream_t stream);",
                 "uint64_t pnr_background_backward_workspace_bytes(uint32_t N);",
                 "int pnr_background_backward(const pnr_background_train_args* args, pnr_stream_t stream);",
                 "int pnr_train_loss_backward_bg(const pnr_train_loss_args* args, float* grad_bg_color /* [N,3] */, pnr_stream_t stream);"):
        assert decl in header, decl
    slab = (64 * 24 + 3 * 64) * 4            # one fp32 slab of both weight gradients per 64 rays
    assert [lib.pnr_background_backward_workspace_bytes(n) for n in (0, 1, 64, 65, 4096)] == [slab, slab, slab, 2 * slab, 64 * slab]


def test_struct_layouts_are_the_headers(tmp_path):
    cname, mirror = "pnr_background_train_args", _lib.BackgroundTrainArgs
    got = c_layout(tmp_path, cname, mirror)
    assert int(got[cname]) == ctypes.sizeof(mirror)
    for fname, *_ in mirror._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, fname
    assert len(mirror._fields_) == 28
    # the structs of ABI 10 did not move (sizes and offsets as the parent commit's header gave them)
    bg = c_layout(tmp_path, "pnr_background_args", _lib.BackgroundArgs)
    assert int(bg["pnr_background_args"]) == ctypes.sizeof(_lib.BackgroundArgs) == 128 and len(_lib.BackgroundArgs._fields_) == 21
    assert [int(bg[f"pnr_background_args.{f}"]) for f in ("N", "rays_o", "coords_in", "table_dtype", "table_rows", "sh_degree", "packed", "coords_out")] \
        == [0, 8, 32, 48, 64, 92, 104, 120]
    tl = c_layout(tmp_path, "pnr_train_loss_args", _lib.TrainLossArgs)
    assert int(tl["pnr_train_loss_args"]) == ctypes.sizeof(_lib.TrainLossArgs) == 240 and len(_lib.TrainLossArgs._fields_) == 36
    assert [int(tl[f"pnr_train_loss_args.{f}"]) for f in ("N", "weights_sum", "bg_color", "bg_const", "bg_mode", "gt_rgb", "lambda_sparsity", "image", "grad_loss",
                                                         "workspace", "workspace_bytes")] == [0, 16, 64, 72, 76, 80, 120, 144, 184, 224, 232]
    for fname, *_ in _lib.TrainLossArgs._fields_:
        assert int(tl[f"pnr_train_loss_args.{fname}"]) == getattr(_lib.TrainLossArgs, fname).offset, fname


@pytest.mark.parametrize("entry, ptrs", [("pnr_background_train_forward", FWD_PTRS), ("pnr_background_backward", BWD_PTRS)])
def test_background_entries_refuse_before_any_launch(entry, ptrs):
    fn = getattr(_lib.load(), entry)
    assert fn(None, None) == INVALID                                                # a null struct
    assert fn(ctypes.byref(_lib.BackgroundTrainArgs()), None) == UNSUPPORTED        # an all-zero architecture
    for field, bad in (("num_levels", 16), ("level_dim", 4), ("sh_degree", 3), ("num_layers", 3), ("hidden_dim", 32), ("gridtype", 2),
                       ("table_dtype", 1),      # an fp16 table: training is fp32
                       ("table_dtype", 2)):
        a = supported(8, ptrs)
        setattr(a, field, bad)
        assert fn(ctypes.byref(a), None) == UNSUPPORTED, field
    assert fn(ctypes.byref(supported(0)), None) == 0                                # N = 0: nothing to do, nothing is read
    assert fn(ctypes.byref(supported(8)), None) == INVALID                          # no pointers at all
    for missing in ptrs:
        if missing == "rays_o":
            continue      # (below: only needed without coords_in)
        a = supported(8, ptrs)
        setattr(a, missing, None)
        assert fn(ctypes.byref(a), None) == INVALID, missing
    a = supported(8, ptrs)
    a.table_rows = 0
    assert fn(ctypes.byref(a), None) == INVALID
    for field in ("coords_in", "embeddings"):
        a = supported(8, ptrs)
        setattr(a, field, 260)
        assert fn(ctypes.byref(a), None) == ALIGNMENT, field


def test_forward_and_backward_specifics():
    lib = _lib.load()
    a = supported(8, FWD_PTRS)
    a.rays_o = None                                  # neither origins nor coordinates
    assert lib.pnr_background_train_forward(ctypes.byref(a), None) == INVALID
    a = supported(8, FWD_PTRS)
    a.coords_out = 260
    assert lib.pnr_background_train_forward(ctypes.byref(a), None) == ALIGNMENT
    a = supported(8, BWD_PTRS)
    a.workspace = 264                                # the slabs are written 16 bytes at a time
    assert lib.pnr_background_backward(ctypes.byref(a), None) == ALIGNMENT
    a = supported(8, BWD_PTRS)
    a.grad_table = 258
    assert lib.pnr_background_backward(ctypes.byref(a), None) == ALIGNMENT
    a = supported(65, BWD_PTRS)
    a.workspace_bytes = lib.pnr_background_backward_workspace_bytes(64)      # one slab short
    assert lib.pnr_background_backward(ctypes.byref(a), None) == INVALID


def test_train_loss_backward_bg_refuses_before_any_launch():
    lib = _lib.load()
    fn = lib.pnr_train_loss_backward_bg
    assert fn(None, 256, None) == INVALID

    def args(n=8, mode=2):
        a = _lib.TrainLossArgs()
        a.N, a.bg_mode = n, mode
        a.weights_sum = a.image_raw = a.gt_rgb = a.bg_color = a.grad_loss = 256
        return a
    for mode in (0, 1):
        assert fn(ctypes.byref(args(mode=mode)), 256, None) == UNSUPPORTED, mode       # a constant or [3] background
    assert fn(ctypes.byref(args(mode=3)), 256, None) == INVALID
    assert fn(ctypes.byref(args(n=0)), 256, None) == 0
    assert fn(ctypes.byref(args()), None, None) == INVALID                             # no place for the gradient
    a = args()
    a.grad_loss = None
    assert fn(ctypes.byref(a), 256, None) == INVALID
    a = args()
    a.bg_color = None
    assert fn(ctypes.byref(a), 256, None) == INVALID
    a = args()
    a.n_channel = 5                                                                    # channels without an all_map
    assert fn(ctypes.byref(a), 256, None) == INVALID


class _Grid2D(torch.nn.Module):
    """A stand-in for encoder_bg on the host (the HIP operators have no CPU form): any differentiable function of the table will do here."""

    def __init__(self, enc):
        super().__init__()
        self.embeddings = enc.embeddings

    def forward(self, x):
        rows = ((x + 1) / 2 * 7).long().clamp(0, 7)
        return torch.cat([self.embeddings[rows[:, 0] * 8 + rows[:, 1] + 8 * l] * x[:, :1] for l in range(4)], dim=-1)


def test_cpu_model_keeps_the_per_op_path(monkeypatch):
    m = network.NeRFNetwork(bound=2, cuda_ray=True, bg_radius=4)
    assert getattr(m, "fused_train_background", True) is True
    m.fused_field, m.march_mode = True, "native"
    with torch.no_grad():
        m.encoder_bg.embeddings.uniform_(-1, 1)
    m.encoder_bg, m.encoder_dir = _Grid2D(m.encoder_bg), TorchSHEncoder(degree=4)
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    g = torch.Generator().manual_seed(0)
    x, d = torch.rand(33, 2, generator=g) * 2 - 1, torch.nn.functional.normalize(torch.randn(33, 3, generator=g), dim=-1)
    assert fused.background_train_fused(m, x, d) is None
    rgb = m.background(x, d)
    rgb.sum().backward()
    assert calls == [] and rgb.shape == (33, 3)
    for p in (m.encoder_bg.embeddings, m.bg_net[0].weight, m.bg_net[1].weight):
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
