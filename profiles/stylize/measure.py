"""Wall time of a 1000-iteration Stylizer fit: the per-op loop (stylize.fit_stylizer_per_op, the only way before pnr_stylizer_fit) against the one
launch, for M = 1, 8, 64 points and nb = 4, 8 bases.  Synchronised, warmed up, `--repeats` timed runs each; prints one JSON line per shape.

    python profiles/stylize/measure.py [--repeats 7] [--iters 1000]
    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/stylize/measure.py --only launch --shape 8 4 --repeats 1 --warmup 0
(the second form: one fit and nothing else on the device, for the launch counts)
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import torch

from palettenerf_amd import renderer, stylize
from tests import stylizer_reference as ref


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--only", choices=("per_op", "launch"))
    ap.add_argument("--shape", type=int, nargs=2, metavar=("M", "NB"))
    a = ap.parse_args()
    device = torch.device("cuda:0")
    shapes = [tuple(a.shape)] if a.shape else [(M, nb) for nb in (4, 8) for M in (1, 8, 64)]
    for M, nb in shapes:
        inp = ref.as_fp32(ref.make_inputs(M, nb, "mild"), device)
        kw = dict(radiance=inp["radiance"], omega=inp["omega"], offsets=inp["offsets"], palette=inp["palette"], colors=inp["target"])

        def launch():
            return stylize.fit_stylizer_from_inputs(**kw, iters=a.iters)

        def per_op():
            st = renderer.Stylizer(types.SimpleNamespace(num_basis=nb)).to(device)
            stylize.fit_stylizer_per_op(st, inp["radiance"], inp["omega"], inp["offsets"], inp["palette"], inp["target"], a.iters, total_iters=a.iters)
            return st

        row = {"M": M, "nb": nb, "iters": a.iters}
        for name, fn in (("per_op", per_op), ("launch", launch)):
            if a.only and a.only != name:
                continue
            ms = timed(fn, a.warmup, a.repeats)
            row[name + "_ms"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "runs": len(ms)}
        if "per_op_ms" in row and "launch_ms" in row:
            row["ratio_of_medians"] = round(row["per_op_ms"]["median"] / row["launch_ms"]["median"], 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
