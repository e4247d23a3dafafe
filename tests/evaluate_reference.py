"""The statements behind pnr_frame_metrics and pnr_palette_sheets (include/pnr.h) as plain torch / numpy, for the tests to compare against.

Meters: every function takes `dtype` -- torch.float64 is the yardstick, torch.float32 is the same text evaluated in single precision (the
error of THAT against float64 is the E of tests/test_gpu_evaluate.py).  Inputs are the fp32 maps the kernels get, converted to `dtype` first.
SSIM is kornia's ssim_loss(window_size=11) with its documented defaults, written out; kornia is not installed where this was written, so the
float64 statement here -- not kornia -- is what the kernel is held to.
Sheets: the numpy expressions of palette/utils.py:993-1038 and :852-909; `(x * 255).astype(np.uint8)` is spelled `.astype(np.int32)
.astype(np.uint8)`, the C conversion `(uint8)(int)` the device performs (numpy's direct float -> uint8 cast is not defined outside 0 .. 255).
"""
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as F

C1, C2, EPS = 0.01 ** 2, 0.03 ** 2, 1e-12
WINDOW, SIGMA = 11, 1.5


def gaussian_window(dtype, device="cpu"):
    x = torch.arange(WINDOW, dtype=dtype, device=device) - (WINDOW // 2)
    g = torch.exp(-(x ** 2) / (2 * SIGMA ** 2))
    g = g / g.sum()
    return g[:, None] * g[None, :]


def srgb_to_linear(x):
    """nerf/utils.py:48-49"""
    return torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def linear_to_srgb_np(x):
    """nerf/utils.py:43-44 in fp32"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x < np.float32(0.0031308), np.float32(12.92) * x, np.float32(1.055) * np.power(x, np.float32(0.41666)) - np.float32(0.055)).astype(np.float32)


def ground_truth(truth, srgb=False, dtype=torch.float64):
    """eval_step, palette/utils.py:617-625: truth [H,W,3 or 4] -> gt_rgb [H,W,3] with bg_color = 1."""
    t = truth.to(dtype)
    rgb = t[..., :3]
    if srgb:
        rgb = srgb_to_linear(rgb)
    if t.shape[-1] == 4:
        return rgb * t[..., 3:] + 1 * (1 - t[..., 3:])
    return rgb


def ssim(pred, gt, eps=EPS):
    """pred, gt [H,W,3] of one dtype -> 1 - 2 * ssim_loss(pred, gt, window_size=11)  (nerf/utils.py:317-318)."""
    p = pred.permute(2, 0, 1)[None]
    t = gt.permute(2, 0, 1)[None]
    k = gaussian_window(p.dtype, p.device).expand(3, 1, WINDOW, WINDOW).contiguous()
    pad = WINDOW // 2

    def filt(z):
        return F.conv2d(F.pad(z, (pad, pad, pad, pad), mode="reflect"), k, groups=3)

    mu1, mu2 = filt(p), filt(t)
    s1 = filt(p * p) - mu1 * mu1
    s2 = filt(t * t) - mu2 * mu2
    s12 = filt(p * t) - mu1 * mu2
    S = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2) + eps)
    return 1 - 2 * torch.clamp((1 - S) / 2, 0, 1).mean()


def sparsity(omega):
    """palette/utils.py:69 ; omega [H,W,nb]"""
    return (omega.sum(dim=-1, keepdim=True) / ((omega ** 2).sum(dim=-1, keepdim=True) + 1e-6) - 1).mean()


def tv(omega):
    """palette/utils.py:101-104"""
    w = torch.mean(torch.pow(omega[:, :-1, :] - omega[:, 1:, :], 2))
    h = torch.mean(torch.pow(omega[:-1, :, :] - omega[1:, :, :], 2))
    return (w + h) * 100


def metrics(pred, truth, basis_acc=None, srgb=False, dtype=torch.float64, device="cpu"):
    """pred [H,W,3], truth [H,W,3 or 4], basis_acc [H,W,nb] or None (fp32 maps) -> {mse, psnr, ssim[, sparsity, tv]} as Python floats."""
    p = pred.to(device).to(dtype)
    gt = ground_truth(truth.to(device), srgb, dtype)
    mse = ((p - gt) ** 2).mean()
    out = {"mse": mse, "psnr": -10 * torch.log10(mse), "ssim": ssim(p, gt)}
    if basis_acc is not None:
        w = basis_acc.to(device).to(dtype)
        out["sparsity"], out["tv"] = sparsity(w), tv(w)
    return {k: float(v.double().cpu()) for k, v in out.items()}


# ---------------------------------------------------------------- sheets
def to_u8(x, clip=True):
    x = np.asarray(x, np.float32)
    if clip:
        x = x.clip(0, 1)
    with np.errstate(invalid="ignore"):
        return (x * np.float32(255)).astype(np.int32).astype(np.uint8)


def sheets(maps, H, W, nb, linear_to_srgb=False):
    """maps: dict of numpy fp32 arrays by ray -- image [HW,3], depth [HW], and optionally view_dep_rgb, direct_rgb [HW,3], basis_rgb,
    unscaled_basis_rgb [HW,3nb], basis_acc, gt_weights [HW,nb], basis_color [nb,3] -> the uint8 images, palette/utils.py:993-1038 / :852-909."""
    out = {}
    pred = maps["image"].reshape(H, W, 3)
    if linear_to_srgb:
        pred = linear_to_srgb_np(pred)
    out["rgb"] = to_u8(pred)
    out["depth"] = to_u8(maps["depth"].reshape(H, W), clip=False)
    for key, name in (("view_dep_rgb", "view_dep"), ("direct_rgb", "direct")):
        if key in maps:
            out[name] = to_u8(maps[key].reshape(H, W, 3))
    for key, name in (("basis_rgb", "basis_img"), ("unscaled_basis_rgb", "unscaled_basis_img")):
        if key in maps:
            out[name] = to_u8(np.concatenate([maps[key][:, i * 3:(i + 1) * 3].reshape(H, W, 3) for i in range(nb)], axis=1))
    if "basis_acc" in maps:
        out["basis_acc"] = to_u8(np.concatenate([maps["basis_acc"][:, i:i + 1].reshape(H, W) for i in range(nb)], axis=1))
    if "gt_weights" in maps:
        g = to_u8(maps["gt_weights"].reshape(H, W, nb))
        out["weights_guide"] = g.transpose(0, 2, 1).reshape(H, -1)
    if "basis_color" in maps:
        sw = [np.tile(maps["basis_color"][i].clip(0, 1)[None, None, :], (100, 100, 1)) for i in range(nb)]
        out["basis_color"] = to_u8(np.concatenate(sw, axis=1))
    return out


# ---------------------------------------------------------------- PNG
def decode_png(path):
    """An 8-bit grey / RGB PNG whose rows all carry filter type 0, decoded with zlib -> uint8 [H,W] or [H,W,3]."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        (n,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, kind
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour, comp, filt, interlace = head
    assert (depth, comp, filt, interlace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    img = rows[:, 1:]
    return img.reshape(h, w, 3).copy() if ch == 3 else img.copy()
