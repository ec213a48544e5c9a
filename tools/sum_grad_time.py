"""A few exact log-prob steps (forward + backward) of the batched exact engine with the sum rbf + locally_periodic + rq and, in the same
process on the same data, with each of its three members alone, at one shape (fp32, n = 8192, q = 8, d = 1, default arithmetic), for a
kernel-trace run of its own: the K^-1 + gradient kernel of each shows as its own row (`k_kinv_grad_add_bf3<..., COV_SUM, 1>` beside
`k_kinv_grad_bf3<...>`, `k_kinv_grad_add_bf3<..., COV_LPER / COV_RQ, 1>`), profiles/sum_grad_kernel_time.md.  The method of
tools/lper_grad_time.py.
`rocprofv3 --kernel-trace --stats -d OUT -- python tools/sum_grad_time.py [--steps 5] [--n 8192]`."""
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
alpha = (1.0 + torch.rand(q, 1, generator=g)).to(dev)
one = torch.ones_like(ell)
lper = torch.stack([1.0 + ell, 0.3 + ell, 4.0 * ell], 1)
members = ["rbf", "locally_periodic", "rq"]
record = lambda e, p, r, al: torch.cat([e, p, r, al], 1)
table = torch.stack([record(ell, one, one, one), record(lper[:, 0], lper[:, 1], lper[:, 2], one), record(2.0 * ell, one, one, alpha)], 1)
cases = {_engine.sum_kind(members): (table, (osc / 3.0).reshape(q, 1).expand(q, 3).contiguous()),
         "rbf": (ell, osc), "locally_periodic": (lper, osc), "rq": (torch.cat([2.0 * ell, alpha], 1), osc)}
out = {}
for kind, (tab, os_) in cases.items():
    for _ in range(a.steps):
        t = tab.clone().requires_grad_()
        lp = _engine.exact_latent_log_prob(kind, X, t, os_, noise, y)
        lp.sum().backward()
    torch.cuda.synchronize()
    out[kind] = float(lp.sum())
print(json.dumps({"n": n, "q": q, "d": d, "steps": a.steps, "logp": out}))
