"""One ProjectedLMCmll training step (forward + backward) with and without `decomp`, HIP-event timed: the numbers of
profiles/additive_engine.txt.  fp32, n = 8192, d = 8, q = 8, p = 16, Matern-5/2, variant PLMC_fast (bench.py's flagship shape).
`python tools/additive_step.py [--decomp 0|1] [--steps 10] [--warmup 3] [--pkg DIR]`; --pkg: a checkout's projected-lmc_amd
directory to import instead of this one (the parent commit's, for the A/B series)."""
import argparse
import json
import os
import sys
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--decomp", type=int, default=1)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--pkg", default=None)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, a.pkg or os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
import projectedlmc as plmc  # noqa: E402

n, d, p, q = a.n, 8, 16, 8
g = torch.Generator().manual_seed(0)
X = 2 * torch.rand(n, d, generator=g) - 1
Y = torch.randn(n, p, generator=g)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    m = plmc.ProjectedGPModel(X, Y, p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True,
                              decomp=[[0, 1, 2, 3], [4, 5, 6, 7]] if a.decomp else None, BDN=True, diagonal_B=True, scalar_B=True)
dev = torch.device("cuda:0")
m = m.to(dev)
Xd, Yd = X.to(dev), Y.to(dev)
m.train(); m.likelihood.train()
mll = plmc.ProjectedLMCmll(m.likelihood, m)


def step():
    for prm in m.parameters():
        prm.grad = None
    loss = -mll(m(Xd), Yd)
    loss.backward()
    return loss


for _ in range(a.warmup):
    step()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.steps):
    loss = step()
e1.record()
torch.cuda.synchronize()
print(json.dumps({"decomp": bool(a.decomp), "pkg": a.pkg or "this", "n": n, "ms_per_step": e0.elapsed_time(e1) / a.steps,
                  "loss": float(loss)}))
