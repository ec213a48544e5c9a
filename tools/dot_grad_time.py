"""A few exact log-prob steps (forward + backward) of the batched exact engine with a dot-product kernel of one power at d = 1 and d = 8
(fp32, n = 8192, q = 8), and -- with --yardstick -- the RBF and the rational-quadratic kernel at the same shapes, for a kernel-trace run
of its own: the K^-1 + gradient kernel of each kind and capacity shows as its own row (`k_kinv_grad_bf3<...>`,
`k_kinv_grad_add_bf3<..., COV_RQ / COV_DOT, 1 / 8>`), profiles/dot_grad_kernel_time.md.  The power is a run-time argument of the kernel,
so one power per process keeps the rows apart.
`rocprofv3 --kernel-trace --stats -d OUT -- python tools/dot_grad_time.py --power 3 [--yardstick] [--steps 5] [--n 8192]`."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--q", type=int, default=8)
ap.add_argument("--power", type=int, default=1)
ap.add_argument("--yardstick", action="store_true")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
from projectedlmc import _engine  # noqa: E402

n, q = a.n, a.q
dev = torch.device("cuda:0")
out = {}
for d in (1, 8):
    g = torch.Generator().manual_seed(d)
    X = (2 * torch.rand(n, d, generator=g) - 1).to(dev)
    y = torch.randn(q, n, generator=g).to(dev)
    v = ((0.3 + 0.7 * torch.rand(q, d, generator=g)) / d).to(dev)
    c = (0.1 + 0.4 * torch.rand(q, 1, generator=g)).to(dev)
    ell = ((0.3 + 0.4 * torch.rand(q, d, generator=g)) * d ** 0.5).to(dev)
    noise = (0.2 + 0.3 * torch.rand(q, generator=g)).to(dev)
    osc = (0.5 + torch.rand(q, generator=g)).to(dev)
    tables = {("linear" if a.power == 1 else "poly%d" % a.power): torch.cat([v, c if a.power > 1 else torch.zeros_like(c)], 1)}
    if a.yardstick:
        tables.update({"rbf": ell, "rq": torch.cat([ell, torch.full((q, 1), 2.0, device=dev)], 1)})
    for kind, table in tables.items():
        for _ in range(a.steps):
            t = table.clone().requires_grad_()
            lp = _engine.exact_latent_log_prob(kind, X, t, osc, noise, y)
            lp.sum().backward()
        torch.cuda.synchronize()
        out["%s d=%d" % (kind, d)] = float(lp.sum())
print(json.dumps({"n": n, "q": q, "power": a.power, "steps": a.steps, "logp": out}))
