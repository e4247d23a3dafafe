"""Figures of the palette weight LUT (profiles/lut/README.md), one MI355X.

  python3 profiles/lut/measure.py [--out FILE]       errors against the longdouble truth and wall times of both legs, profiler off: JSON lines
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o lut -- python3 profiles/lut/measure.py --once
                                                      one weight_lut per palette (M = 4, 6, 8; plain and normalised) under the tracer

Palettes: the fixtures of tests/lut_reference.py at N = 32 768 (the five-bit bins).  The host leg is extract.weight_lut_per_op, the same statement
in numpy float64, timed in the same process; the reference's own loop (scipy, cvxopt, a Cython module) does not import here and is not timed."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from palettenerf_amd import extract  # noqa: E402
from tests import lut_reference as ref  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    cuda = torch.device("cuda:0")
    if "--once" in sys.argv:
        for name, norm in ref.FIXTURES:
            extract.weight_lut(ref.PALETTES[name], normalize_input=norm, device=cuda)
        torch.cuda.synchronize()
        print(json.dumps({"launches": len(ref.FIXTURES)}))
        return
    lines = []
    for name, norm in ref.FIXTURES:
        palette = ref.PALETTES[name]
        truth, info = ref.truth(name, norm)
        (lut, w64), _ = timed(lambda: extract.weight_lut(palette, normalize_input=norm, device=cuda, return_weights64=True))      # warm-up
        host = extract.weight_lut_per_op(palette, normalize_input=norm)
        w = w64.cpu().numpy()
        rec = {"palette": name, "M": int(palette.shape[0]), "normalize_input": norm, "outside": int(info["outside"].sum()), "faces": int(len(info["faces"])),
               "kernel_error": float(np.abs(w - truth).max()), "per_op_error": float(np.abs(host.reshape(-1, host.shape[-1]) - truth).max()),
               "kernel_equals_per_op_bits": bool(np.array_equal(w, host.reshape(-1, host.shape[-1]))),
               "device_ms": [], "device_event_ms": [], "per_op_ms": []}
        for _ in range(5):                                                              # legs alternating
            rec["device_ms"].append(timed(lambda: extract.weight_lut(palette, normalize_input=norm, device=cuda))[1])
            t0 = time.perf_counter()
            extract.weight_lut_per_op(palette, normalize_input=norm)
            rec["per_op_ms"].append((time.perf_counter() - t0) * 1e3)
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            extract.weight_lut(palette, normalize_input=norm, device=cuda)
            e1.record()
            torch.cuda.synchronize()
            rec["device_event_ms"].append(e0.elapsed_time(e1))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
