"""A few exact log-prob steps (forward + backward) of the batched exact engine with the Matern-5/2, the periodic and the locally periodic
kernel at one shape (fp32, n = 8192, q = 8, d = 1), for a kernel-trace run of its own: the K^-1 + gradient kernel of each kind shows as
its own row (`k_kinv_grad_bf3<...>`, `k_kinv_grad_add_bf3<..., COV_PER / COV_LPER, 1>`), profiles/lper_grad_kernel_time.md.  The method
of tools/rq_grad_time.py.
`rocprofv3 --kernel-trace --stats -d OUT -- python tools/lper_grad_time.py [--steps 5] [--n 8192]`."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--q", type=int, default=8)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
from projectedlmc import _engine  # noqa: E402

n, q, d = a.n, a.q, 1
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
X = torch.sort(torch.rand(n, d, generator=g), 0)[0].to(dev)
y = torch.randn(q, n, generator=g).to(dev)
ell = (0.05 + 0.1 * torch.rand(q, d, generator=g)).to(dev)
noise = (0.05 + 0.1 * torch.rand(q, generator=g)).to(dev)
osc = (0.5 + torch.rand(q, generator=g)).to(dev)
tables = {"matern52": ell,
          "periodic": torch.stack([1.0 + ell, 0.3 + ell], 1),
          "locally_periodic": torch.stack([1.0 + ell, 0.3 + ell, 4.0 * ell], 1)}
out = {}
for kind, table in tables.items():
    for _ in range(a.steps):
        t = table.clone().requires_grad_()
        lp = _engine.exact_latent_log_prob(kind, X, t, osc, noise, y)
        lp.sum().backward()
    torch.cuda.synchronize()
    out[kind] = float(lp.sum())
print(json.dumps({"n": n, "q": q, "d": d, "steps": a.steps, "logp": out}))
