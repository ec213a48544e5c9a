"""One ProjectedLMCmll training step (forward + backward) with the spectral-mixture kernel beside the Matern-5/2 one, HIP-event
timed: the step times of profiles/sm_resource_usage.md.  fp32, n = 8192, q = 8, p = 16, d = 1, M = 5 (bench.py's flagship size on the
one-dimensional input of the reference's tidal study).  `python tools/sm_step.py [--sm 0|1] [--mixtures 5] [--steps 10] [--warmup 3]`."""
import argparse
import json
import os
import sys
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--sm", type=int, default=1)
ap.add_argument("--mixtures", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--n", type=int, default=8192)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
import projectedlmc as plmc  # noqa: E402

n, d, p, q = a.n, 1, 16, 8
g = torch.Generator().manual_seed(0)
X = torch.sort(torch.rand(n, d, generator=g), 0)[0]
Y = torch.randn(n, p, generator=g)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    kw = dict(kernel_type=plmc.SpectralMixtureKernel, ker_kwargs={"num_mixtures": a.mixtures}) if a.sm else dict(kernel_type=plmc.MaternKernel)
    m = plmc.ProjectedGPModel(X, Y, p, q, mean_type=plmc.ZeroMean, init_lmc_coeffs=True, BDN=True, diagonal_B=True, scalar_B=True, **kw)
if a.sm:
    m.covar_module.initialize_from_data(X, Y)
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
print(json.dumps({"kernel": "spectral mixture, M = %d" % a.mixtures if a.sm else "matern52", "n": n, "q": q, "d": d,
                  "ms_per_step": e0.elapsed_time(e1) / a.steps, "loss": float(loss)}))
