"""Figures of the hull simplification (profiles/hull/README.md), one MI355X.

  python3 profiles/hull/measure.py [--out FILE]      E, the kernel's error against the longdouble truth on every fixture, and wall times of
                                                      both legs on mix(2, 44), shell(11) and the 128 shell points, profiler off: JSON lines
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o hull -- python3 profiles/hull/measure.py --once
                                                      one simplify_hull per case under the tracer

The host leg is extract.simplify_hull_per_op (scipy's ConvexHull and linprog(method="highs") in the reference's line order), timed in the same
process; the reference's own function (cvxopt/GLPK, a Cython module, its trimesh.py) does not import here and is not timed."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from palettenerf_amd import extract  # noqa: E402
from tests import hull_reference as ref  # noqa: E402

CASES = (("mix-2-44", lambda: ref.fixture("mix-2-44")), ("shell-11", lambda: ref.fixture("shell-11")), ("shell-128", ref.shell128))


def main():
    if "--once" in sys.argv:
        for name, make in CASES:
            c, w = make()
            extract.simplify_hull(c, w)
        torch.cuda.synchronize()
        print(json.dumps({"launches": len(CASES)}))
        return
    lines = []
    E = ref.fixture_E()
    worst = 0.0
    for name in ref.NAMES:
        t = ref.truth(name)
        if t["status"] != ref.OK:
            continue
        palette, info = extract.simplify_hull(*ref.fixture(name), return_info=True)
        err = float(np.max(np.abs(palette - t["palette"])))
        err_host = float(np.max(np.abs(ref.host(name)[0] - t["palette"])))
        worst = max(worst, err)
        lines.append({"fixture": name, "initial": info["initial"], "M": info["M"], "collapses": info["collapses"], "related": info["related"],
                      "kernel_error": err, "host_formulation_error": err_host})
        print(json.dumps(lines[-1]), flush=True)
    lines.append({"E": E, "kernel_error_max": worst, "kernel_over_E": worst / E})
    print(json.dumps(lines[-1]), flush=True)
    for name, make in CASES:
        c, w = make()
        extract.simplify_hull(c, w)                                                     # warm-up
        rec = {"case": name, "K": int(c.shape[0]), "device_ms": [], "per_op_ms": []}
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            palette, info = extract.simplify_hull(c, w, return_info=True)
            rec["device_ms"].append((time.perf_counter() - t0) * 1e3)
        rec.update(initial=info["initial"], M=info["M"], collapses=info["collapses"], related=info["related"])
        for _ in range(1 if c.shape[0] > 64 else 2):
            t0 = time.perf_counter()
            host = extract.simplify_hull_per_op(c, w)
            rec["per_op_ms"].append((time.perf_counter() - t0) * 1e3)
        rec["device_minus_per_op"] = float(np.max(np.abs(palette - host)))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
