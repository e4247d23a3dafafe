"""Figures of the coloured mesh export (profiles/mesh_color/README.md), one MI355X.

  python3 profiles/mesh_color/mesh_color_profile.py [--out FILE]     wall times, profiler off: one JSON line
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mesh_color -- python3 profiles/mesh_color/mesh_color_profile.py --once
                                                                      one fused and one per-op gradient call on the same 2^20 points, under the tracer

Fields: bench.py's synthetic fields, scene.seed_field_(..., 0) at bound 2 -- a NeRFNetwork for the gradient, a PaletteNetwork (4 bases) for save_mesh."""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from palettenerf_amd import mesh, network, renderer, scene  # noqa: E402

N = 1 << 20


def wall(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def gradient_figures(cuda, once):
    m = scene.seed_field_(network.NeRFNetwork(bound=2, cuda_ray=True, density_scale=1), 0).to(cuda).eval()
    pts = ((torch.rand(N, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 2).to(cuda)
    assert m._fused_sweep_ok()
    if once:
        mesh.density_gradient(m, pts)
        torch.cuda.synchronize()
        mesh.density_gradient_per_op(m, pts)
        torch.cuda.synchronize()
        return {}
    fused = wall(lambda: mesh.density_gradient(m, pts))
    normal_only = wall(lambda: mesh.density_gradient(m, pts, want=("normal",)))
    per_op = wall(lambda: mesh.density_gradient_per_op(m, pts))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mesh.density_gradient_per_op(m, pts)
    torch.cuda.synchronize()
    peak_per_op = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mesh.density_gradient(m, pts)
    torch.cuda.synchronize()
    peak_fused = torch.cuda.max_memory_allocated() - base
    return {"points": N, "fused_ms": fused, "fused_normal_only_ms": normal_only, "per_op_ms": per_op, "per_op_peak_extra_bytes": int(peak_per_op),
            "fused_peak_extra_bytes": int(peak_fused), "dy_dx_bytes": N * 16 * 3 * 2 * 4}


def stage(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def save_mesh_figures(cuda, R=256):
    nb = 4
    m = scene.seed_field_(network.PaletteNetwork(renderer.default_opt(num_basis=nb), bound=2, cuda_ray=True, density_scale=1), 0).to(cuda).eval()
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    u = mesh.lattice_density(m, lo, hi, R)
    median = float(u.median())
    del u
    out = {"resolution": R, "median": median}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mesh.ply")
        mesh.save_mesh(m, path, R, 10, attributes="palette")                    # warm-up: first use of every kernel
        for name, thr in (("threshold_10", 10.0), ("threshold_median", median)):
            row = {"threshold": thr}
            u, row["density_ms"] = stage(lambda: mesh.lattice_density(m, lo, hi, R))
            (v, t), row["surface_ms"] = stage(lambda: mesh.marching_cubes(u, thr))
            del u

            def attributes():
                world, _ = mesh.vertex_records(v, lo, hi, R, want_records=False)
                a = mesh.vertex_attributes(m, world)
                nv = v.shape[0]
                extra = torch.cat([a["radiance"].reshape(nv, 1), a["omega"].reshape(nv, nb), a["offsets"].reshape(nv, 3 * nb)], dim=1).contiguous()
                return mesh.vertex_records(v, lo, hi, R, normal=a["normal"], rgb=a["base_rgb"], extra=extra)[1]

            rec, row["attributes_ms"] = stage(attributes)
            (rec_h, t_h), row["read_back_ms"] = stage(lambda: (rec.cpu().numpy(), t.cpu().numpy()))
            props = mesh.XYZ_PROPERTIES + mesh.NORMAL_PROPERTIES + mesh.RGBA_PROPERTIES + mesh.palette_properties(nb)
            _, row["file_ms"] = stage(lambda: mesh.write_ply(path, None, t_h, records=rec_h, properties=props))
            row["vertices"], row["triangles"], row["ply_bytes"] = int(v.shape[0]), int(t.shape[0]), os.path.getsize(path)
            del rec, rec_h, t_h, v, t
            torch.cuda.empty_cache()
            _, row["save_mesh_ms"] = stage(lambda: mesh.save_mesh(m, path, R, thr, attributes="palette"))
            _, row["save_mesh_plain_ms"] = stage(lambda: mesh.save_mesh(m, path, R, thr))
            out[name] = row
            print(name, json.dumps(row), flush=True)
    return out


def main():
    cuda = torch.device("cuda:0")
    once = "--once" in sys.argv
    res = {"gradient": gradient_figures(cuda, once)}
    if not once:
        print(json.dumps(res), flush=True)
        res["save_mesh"] = save_mesh_figures(cuda)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
