"""How many distinct 128-byte table lines a gather instruction of the frame loop's lookup asks for, counted on the CPU -- no GPU needed.

The input is the 128x128 centre region of pose 0 of bench.py's lego workload at full resolution, rays in 8x8 tile order (one wave = one tile while
n_step is 1).  The positions are the CPU oracle's: the repository's renderer runs its per-op loop with the oracle's march / composite and torch's
CPU MLP, and the march calls of iterations 0, 5, 15 and 25 are recorded.  Row indices follow oracle/torch_encoders.py's arithmetic (dense or hashed
per level, `%` by the level's size); a line is 128 bytes of the fp32 table, absolute (level offset included).

Per level and iteration, summed over the 8 gather instructions of a wave and averaged over the waves:
  lane = sample      today's mapping: instruction c fetches corner c of the lanes' 64 samples
  lane pair = x-pair the lane-pair form (frame.hip: grid_pair_level): lanes 2k, 2k+1 fetch corners (x, y+j, z+k) / (x+1, y+j, z+k) of sample 2k in
                     instructions 0..3 and of sample 2k+1 in instructions 4..7
  whole wave         distinct lines over all 512 rows of the wave (what an infinite L1 would fetch)
and, as a second model of the texture path, a quad of lanes costing one cycle per distinct line (max 4).

usage: python profiles/grid_line_sharing.py [--crop 128] [--iterations 0 5 15 25]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = 128
ROW_BYTES = 8
_P1, _P2, _M32 = 2654435761, 805459861, 0xFFFFFFFF


def record_positions(crop, iterations):
    """-> {iteration: (x in [0,1]^3 [rows, 3], live [rows])} of the oracle-driven frame loop, rays in 8x8 tile order"""
    import bench
    import oracle
    from oracle.facade import make_oracle_modules
    from palettenerf_amd import renderer, scene
    from palettenerf_amd.fused import tile_ray_order
    import palettenerf_amd.gridencoder as pge
    import palettenerf_amd.shencoder as psh
    args = bench.parse(["--workload", "lego"])
    H, W = args.wl["H"], args.wl["W"]
    pose = torch.from_numpy(bench.pose_of(args, 0)[None])
    ro, rd = scene.get_rays(pose, bench.intrinsics_of(args), H, W)
    idx = bench.crop_indices(H, W, crop)
    idx = idx[tile_ray_order(torch.arange(crop * crop), crop, 8).long()]
    ro, rd = ro[:, idx].contiguous(), rd[:, idx].contiguous()
    rm, ge, sh, _ = make_oracle_modules()
    seen, calls = {}, [0]
    inner = rm.march_rays

    def march_rays(n_alive, n_step, *a, **k):
        x, d, dl = inner(n_alive, n_step, *a, **k)
        if calls[0] in iterations:
            rows = n_alive * n_step
            seen[calls[0]] = (x[:rows].numpy().copy(), dl[:rows, 0].numpy() != 0, n_step)
        calls[0] += 1
        return x, d, dl

    rm.march_rays = march_rays
    saved = (renderer.raymarching, pge.GridEncoder, psh.SHEncoder)
    renderer.raymarching, pge.GridEncoder, psh.SHEncoder = rm, ge.GridEncoder, sh.SHEncoder
    try:
        m = bench.make_model(args, "nerf")
        scene.seed_field_(m, 0)
        grid = bench.density_grid_of(args.wl["scene"])
        m.density_grid.copy_(torch.from_numpy(grid))
        m.density_bitfield.copy_(torch.from_numpy(oracle.packbits(grid, 0.5)))
        m.eval()
        with torch.no_grad():
            m.render(ro, rd, perturb=False, dt_gamma=args.wl["dt_gamma"], max_steps=1024, T_thresh=1e-4)
        bound, enc = float(m.bound), m.encoder
        offs = [int(o) for o in enc.offsets.tolist()]
        scale, res = oracle.grid_level_params(len(offs) - 1, enc.per_level_scale, enc.base_resolution)
    finally:
        renderer.raymarching, pge.GridEncoder, psh.SHEncoder = saved
    out = {}
    for it, (x, live, n_step) in seen.items():
        out[it] = ((x + bound) / (2 * bound), live, n_step)
    return out, offs, [float(s) for s in scale], [int(r) for r in res], calls[0]


def corner_lines(x, offs, scale, res, lv):
    """line index [rows, 8] of the eight corner rows of every sample on level lv (corner c: bit d of c = +1 in dimension d)"""
    size, side = offs[lv + 1] - offs[lv], res[lv] + 1
    pos = x.astype(np.float32) * np.float32(scale[lv]) + np.float32(0.5)
    pg = np.floor(pos).astype(np.int64).clip(min=0)
    dense = side ** 3 <= size
    lines = np.empty((x.shape[0], 8), np.int64)
    for c in range(8):
        p = [pg[:, d] + ((c >> d) & 1) for d in range(3)]
        if dense:
            index = p[0] + p[1] * side + p[2] * (side * side)
        else:
            index = (p[0] & _M32) ^ ((p[1] * _P1) & _M32) ^ ((p[2] * _P2) & _M32)
        lines[:, c] = ((offs[lv] + index % size) * ROW_BYTES) // LINE
    return lines


def per_instruction(lines_by_lane):
    """lines_by_lane [64] (-1 = the lane loads nothing) -> (distinct lines, quad cycles: one per distinct line of every 4 lanes)"""
    v = lines_by_lane[lines_by_lane >= 0]
    quads = 0
    for q in range(0, 64, 4):
        s = lines_by_lane[q:q + 4]
        quads += len(set(s[s >= 0].tolist()))
    return len(set(v.tolist())), quads


def count(lines, live):
    """lines [rows, 8], live [rows] -> per-wave means: (today lines, pair lines, wave lines, today quad cycles, pair quad cycles)"""
    rows = lines.shape[0]
    pad = (-rows) % 64
    lines = np.concatenate([lines, np.full((pad, 8), -1, np.int64)])
    live = np.concatenate([live, np.zeros(pad, bool)])
    lines[~live] = -1
    tot = np.zeros(5)
    n_waves = 0
    for w0 in range(0, lines.shape[0], 64):
        wl = lines[w0:w0 + 64]
        if not (wl >= 0).any():
            continue
        n_waves += 1
        for c in range(8):                                   # today: instruction c = corner c of every lane's own sample
            a, b = per_instruction(wl[:, c])
            tot[0] += a; tot[3] += b
        for half in range(2):                                # pairs: instructions 0..3 serve the even sample of a pair, 4..7 the odd one
            for jk in range(4):
                by_lane = np.empty(64, np.int64)
                by_lane[0::2] = wl[half::2, 2 * jk]          # even lane: the (x, ..) corner
                by_lane[1::2] = wl[half::2, 2 * jk + 1]      # odd lane: the (x + 1, ..) corner of the same cell
                a, b = per_instruction(by_lane)
                tot[1] += a; tot[4] += b
        tot[2] += len(set(wl[wl >= 0].tolist()))
    return tot / max(n_waves, 1), n_waves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--iterations", type=int, nargs="*", default=[0, 5, 15, 25])
    a = ap.parse_args()
    seen, offs, scale, res, n_iter = record_positions(a.crop, set(a.iterations))
    print(f"# lego pose 0, centre {a.crop}x{a.crop}, 8x8 tile order; the oracle's loop ran {n_iter} iterations; lines of {LINE} bytes, rows of {ROW_BYTES}")
    for it in sorted(seen):
        x, live, n_step = seen[it]
        print(f"\niteration {it}: {x.shape[0]} rows (n_step {n_step}), {live.mean() * 100:.1f} % live")
        print(f"{'level':>5} {'lane = sample':>14} {'lane pair':>10} {'whole wave':>11} {'quad cycles':>12} {'pair quad cycles':>17}")
        sums = np.zeros(5)
        for lv in range(len(offs) - 1):
            t, _ = count(corner_lines(x, offs, scale, res, lv), live)
            sums += t
            print(f"{lv:5d} {t[0]:14.1f} {t[1]:10.1f} {t[2]:11.1f} {t[3]:12.1f} {t[4]:17.1f}")
        print(f"  all {sums[0]:14.1f} {sums[1]:10.1f} {sums[2]:11.1f} {sums[3]:12.1f} {sums[4]:17.1f}    pair / today: {sums[1] / sums[0]:.2f} in lines, {sums[4] / sums[3]:.2f} in quad cycles")


if __name__ == "__main__":
    main()
