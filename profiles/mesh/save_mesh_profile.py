"""A 256^3 mesh export of bench.py's synthetic lego field (scene.seed_field_(NeRFNetwork(bound=2), 0)), for profiles/mesh/README.md.

    python3 profiles/mesh/save_mesh_profile.py                      # wall times (device-synchronised host clock)
    rocprofv3 --kernel-trace --stats -d DIR -o mesh -- python3 profiles/mesh/save_mesh_profile.py --once      # kernel times, a run of its own

The seeded field has no object in it -- its density is exp(small) everywhere -- so the reference's threshold 10 gives an empty mesh; the export is
timed at that threshold and at the volume's median, where half the lattice is inside and the surface is as large as this field makes it.
One full occupancy sweep (pnr_occupancy_update, 2 x 128^3 samples) runs in the same process: the same lookup and sigma_net arithmetic."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from palettenerf_amd import mesh, network, scene     # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--once", action="store_true", help="one pass of everything (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1, min_near=0.2)
    scene.seed_field_(m, 0)
    m = m.to(dev).eval()
    R, reps = args.resolution, 1 if args.once else 5
    res = {"resolution": R}
    if not args.once:                                   # warm every shape the timed window uses
        m.update_extra_state()
        u = mesh.lattice_density(m, resolution=R)
        mesh.marching_cubes(u, float(u.median()))
    _, res["occupancy_update_ms"] = timed(lambda: m.update_extra_state(), reps)
    res["occupancy_samples"] = m.cascade * m.grid_size ** 3
    u, res["lattice_density_ms"] = timed(lambda: mesh.lattice_density(m, resolution=R), reps)
    median = float(u.median())
    res["u_min_median_max"] = [float(u.min()), median, float(u.max())]
    for name, thr in (("threshold_10", 10.0), ("threshold_median", median)):
        (v, t), ms = timed(lambda: mesh.marching_cubes(u, thr), reps)
        res[name] = {"threshold": thr, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "marching_cubes_ms": ms}
        with tempfile.TemporaryDirectory() as d:
            _, ms = timed(lambda: mesh.save_mesh(m, os.path.join(d, "mesh.ply"), resolution=R, threshold=thr), 1 if args.once else 2)
            res[name]["save_mesh_ms"] = ms
            res[name]["ply_bytes"] = os.path.getsize(os.path.join(d, "mesh.ply"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
