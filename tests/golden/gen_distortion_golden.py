"""Writes tests/golden/distortion_effdist.npz: a recorded run of the reference's own EffDistLoss (loss.py:29-76), imported from a reference
checkout at generation time only (the fixture it writes is data; no test reads the checkout).

8 rays x 24 samples in float64: volume-rendering weights w of random densities, midpoints m, intervals, the loss (EffDistLoss divides the
sum over rays by n_rays = 8) and d loss / d w from its hand-written backward.  tests/test_distortion_host.py holds
tests/distortion_reference.py's float64 statement to these numbers.

    python tests/golden/gen_distortion_golden.py [path of the reference checkout]"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "distortion_effdist.npz")


def main():
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(REF, "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(2024)
    B, K = 8, 24
    interval = rng.uniform(0.004, 0.05, (B, K))
    sigma = rng.random((B, K)) * 40 * np.where(rng.random((B, 1)) < 0.5, 0.1, 1.0)
    alpha = 1 - np.exp(-sigma * interval)
    T = np.concatenate([np.ones((B, 1)), np.cumprod(1 - alpha, -1)[:, :-1]], -1)
    w = alpha * T
    m = rng.uniform(2.0, 6.0, (B, 1)) + np.cumsum(interval * rng.uniform(0.9, 1.1, (B, K)), -1)
    wt = torch.tensor(w, requires_grad=True)
    loss = ref.eff_distloss(wt, torch.tensor(m), torch.tensor(interval))
    loss.backward()
    np.savez(OUT, w=w, m=m, interval=interval, loss=np.float64(loss.item()), grad_w=wt.grad.numpy())
    print(f"wrote {OUT}: loss {loss.item():.17g}")


if __name__ == "__main__":
    main()
