"""How tests/stylizer_reference.py:SEEDS was chosen -- on the CPU, no kernel involved.  For every long-run case of tests/test_gpu_stylize.py and
seeds 0, 1, 2, ...: E = deviation of the fp32 per-op loop from the float64 loop, A = deviation of the reference module's analytic-gradient loop
run in fp32.  The first seed with E <= 2.5e-4 and E / 2 <= A <= 2 E is taken.

    python profiles/stylize/seed_scan.py [--seeds 12]
"""
import argparse
import os
import sys
import types

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

from palettenerf_amd import renderer, stylize
from tests import stylizer_reference as ref

CASES = [(1, 4, "mild", False), (3, 4, "mild", False), (5, 8, "mild", False), (3, 4, "hard", False), (17, 5, "hard", False), (64, 4, "hard", False),
         (17, 5, "hard", True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=12)
    a = ap.parse_args()
    chosen = {}
    for M, nb, regime, vd in CASES:
        for seed in range(a.seeds):
            inp64, want, _, _ = ref.reference_run(M, nb, regime, view_dep=vd, seed=seed)
            inp = ref.as_fp32(inp64)
            st = renderer.Stylizer(types.SimpleNamespace(num_basis=nb))
            stylize.fit_stylizer_per_op(st, inp["radiance"], inp["omega"], inp["offsets"], inp["palette"], inp["target"], 1000, view_dep=inp["view_dep"])
            E = ref.deviation(stylize._params(st), want)
            A = ref.deviation(ref.sgd(inp, 1000, total_iters=1000, analytic=True)[0], want)
            ok = E <= 2.5e-4 and E / 2 <= A <= 2 * E
            print(f"M={M} nb={nb} {regime} view_dep={vd} seed={seed}: per-op E={E:.3e} analytic fp32 A={A:.3e} {'<- taken' if ok else ''}", flush=True)
            if ok:
                chosen[(M, nb, regime, vd, 1000)] = seed
                break
    print("SEEDS =", chosen)


if __name__ == "__main__":
    main()
