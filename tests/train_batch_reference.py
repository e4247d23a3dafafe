"""What a training step does in front of model.render, restated twice (the reference's provider and trainer cannot be imported: cv2 and
tensorboardX are absent), as tests/evaluate_reference.py does for the evaluate loops:

  * numpy float64 -- the yardstick: `collate` (palette/provider.py:356-410), the head of train_step (palette/utils.py:459-478 with
    nerf/utils.py:48-49 and palette/utils.py:117-124) and the error-map update (palette/utils.py:578-599);
  * torch fp32 -- the same expressions as the reference writes them (torch.gather, rand_like's blend, grid_sample behind the [2,1,0] swizzle,
    gather / scatter_), on whatever device the inputs live on.  Their distance from float64 is the E of the 4 x E bounds.
"""
import numpy as np
import torch


# ---------------------------------------------------------------- storage

def decode(stack):
    """A stored stack as the fp32 values the loader would hold: uint8 -> astype(float32) / 255 (provider.py: `image.astype(np.float32) / 255`),
    fp16 -> exact conversion, fp32 as is.  numpy in, numpy out."""
    if stack.dtype == np.uint8:
        return stack.astype(np.float32) / 255
    return stack.astype(np.float32)


# ---------------------------------------------------------------- float64

def gather_f64(stack, view_index, inds):
    """collate's pixel gather: stack [V,H,W,C] (decoded fp32), view_index [B], inds [B,N] -> [B,N,C] float64."""
    V, H, W, C = stack.shape
    flat = stack.reshape(V, H * W, C).astype(np.float64)
    return np.stack([flat[v][i] for v, i in zip(np.asarray(view_index), np.asarray(inds))])


def srgb_to_linear_f64(x):
    x = np.asarray(x, np.float64)
    return np.where(x < 0.04045, x / 12.92, ((np.maximum(x, 0) + 0.055) / 1.055) ** 2.4)     # nerf/utils.py:48-49


def blend_f64(pixels, bg, linear=False):
    """train_step:459-473: pixels [...,C] fp64, bg a number, [3] or [...,3] -> gt_rgb [...,3]."""
    rgb = np.asarray(pixels[..., :3], np.float64)
    if linear:
        rgb = srgb_to_linear_f64(rgb)
    if pixels.shape[-1] == 3:
        return rgb
    a = np.asarray(pixels[..., 3:], np.float64)
    return rgb * a + np.asarray(bg, np.float64) * (1 - a)


def lut_f64(rgb, hist):
    """get_palette_weight_with_hist (palette/utils.py:117-124) as one sentence: hist[k, r, g, b] read trilinearly at c (S - 1) per channel, corners
    at an index outside [0, S) count as zero (padding_mode='zeros', align_corners=True; the [2,1,0] swizzle maps r to the slowest axis).
    rgb [...,3], hist [nb,Sr,Sg,Sb] -> [...,nb] float64."""
    rgb = np.asarray(rgb, np.float64)
    hist = np.asarray(hist, np.float64)
    nb, S = hist.shape[0], hist.shape[1:]
    flat = rgb.reshape(-1, 3)
    x = [flat[:, c] * (S[c] - 1) for c in range(3)]
    i0 = [np.floor(v).astype(np.int64) for v in x]
    f = [v - i for v, i in zip(x, i0)]
    out = np.zeros((flat.shape[0], nb))
    for dr in (0, 1):
        for dg in (0, 1):
            for db in (0, 1):
                idx = [i0[0] + dr, i0[1] + dg, i0[2] + db]
                w = (f[0] if dr else 1 - f[0]) * (f[1] if dg else 1 - f[1]) * (f[2] if db else 1 - f[2])
                ok = np.ones(flat.shape[0], bool)
                for c in range(3):
                    ok &= (idx[c] >= 0) & (idx[c] < S[c])
                ii = [np.clip(idx[c], 0, S[c] - 1) for c in range(3)]
                out += np.where(ok, w, 0.0)[:, None] * hist[:, ii[0], ii[1], ii[2]].T
    return out.reshape(*rgb.shape[:-1], nb)


def error_map_f64(error_map, view_index, inds_coarse, loss_ray):
    """palette/utils.py:583-599 on a copy: map[v, c] = 0.1 map[v, c] + 0.9 loss (unique cells per view)."""
    m = np.array(error_map, np.float64)
    for b, v in enumerate(np.asarray(view_index)):
        c = np.asarray(inds_coarse)[b]
        m[v, c] = 0.1 * m[v, c] + 0.9 * np.asarray(loss_ray, np.float64)[b]
    return m


# ---------------------------------------------------------------- torch fp32, as the reference writes it

def collate_torch(images, view_index, inds):
    """provider.py:392-395 (and :399-402 for feat_images): images [V,H,W,C] torch (any float dtype), view_index [B], inds [B,N] -> [B,N,C]."""
    B = view_index.shape[0]
    sel = images[view_index]
    C = sel.shape[-1]
    return torch.gather(sel.view(B, -1, C), 1, torch.stack(C * [inds], -1))


def srgb_to_linear_torch(x):
    return torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def head_torch(images, bg_color, linear=False):
    """train_step:457-473 on the gathered pixels [B,N,C] (a clone: the reference writes the linear colours in place)."""
    images = images.clone()
    C = images.shape[-1]
    if linear:
        images[..., :3] = srgb_to_linear_torch(images[..., :3])
    if C == 4:
        return images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
    return images


def lut_torch(rgb, hist_weights):
    """palette/utils.py:117-124 (its squeeze() written as a reshape, so that one ray works too); hist_weights [1,nb,Sr,Sg,Sb]."""
    assert hist_weights.ndim == 5
    rgb_shape = rgb.shape
    rgb = rgb.reshape(-1, 3)
    rgb = rgb[None, None, None, :, [2, 1, 0]] * 2 - 1
    weight = torch.nn.functional.grid_sample(hist_weights, rgb, mode="bilinear", padding_mode="zeros", align_corners=True)
    weight = weight.reshape(hist_weights.shape[1], -1).permute(1, 0)
    return weight.reshape(rgb_shape[:-1] + (-1,))


def error_map_torch(error_map, index, inds, loss):
    """palette/utils.py:583-599 on the given map (in place, as the reference)."""
    rows = error_map[index]
    ema = 0.1 * rows.gather(1, inds) + 0.9 * loss
    rows.scatter_(1, inds, ema)
    error_map[index] = rows
    return error_map


def parent_batch(poses, intrinsics, H, W, N, images, view_index, hist_weights=None, error_map=None, patch_size=1, random_size=0, linear=False,
                 random_bg=True):
    """A training batch the way the tree formed one before TrainSet: rays.get_rays plus the expressions above, RNG calls in the reference's order."""
    from palettenerf_amd import rays
    emap = None if error_map is None else error_map[view_index]
    r = rays.get_rays(poses[view_index], intrinsics, H, W, N, emap, patch_size, random_size)
    px = collate_torch(images, view_index, r["inds"]).float()
    bg = torch.rand_like(px[..., :3]) if (px.shape[-1] == 4 and random_bg) else 1
    gt = head_torch(px, bg, linear)
    gw = lut_torch(gt, hist_weights) if hist_weights is not None else None
    return dict(r, pixels=px, bg_color=bg, gt_rgb=gt, gt_weights=gw)
