"""Time of plmc_cross_matvec_dx_f32 at the metric shape (n = 8192, q = 8, d = 8, Matern-5/2, fp32), n* in {64, 2048}, r in {1, 8}, beside
the composed route the parent commit offers for the same gradient -- torch.bmm forming B = V G^T (q n n* values) followed by
plmc_posterior_dx_f32, whose Jv is -2 sum_i B_is d k: the same derivative up to the factor -2 -- and beside plmc_cross_matvec_f32 (the
values) at the same shape.  Device events around every call, median of --reps calls after 3 warm-up calls, the routes alternating call by
call in one process.
`python tools/cross_matvec_dx_time.py [--md profiles/cross_matvec_dx_time.md] [--n 8192] [--reps 20]`"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--md", default=None)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
from projectedlmc import _engine, _hip  # noqa: E402

assert torch.cuda.is_available(), "tools/cross_matvec_dx_time.py measures on the GPU only"
dev = torch.device("cuda:0")
dt = torch.float32
n, q, d = a.n, 8, 8
WARM = 3


def timed(fns, reps):
    """Median ms of each callable, alternating them call by call."""
    for _ in range(WARM):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


g = torch.Generator().manual_seed(0)
X = (2 * torch.rand(n, d, generator=g) - 1).to(dev)
ell = (0.6 + 0.8 * torch.rand(q, d, generator=g)).to(dev)
alpha = torch.zeros(q, n, device=dev)
L = _hip.lib().cdll
lines = ["| n* | r | ranges (`plmc_cross_matvec_dx_splits`) | `plmc_cross_matvec_dx_f32` | composed: `torch.bmm` (V G^T, q n n* values) + `plmc_posterior_dx_f32` "
         "(its ranges) | of which `torch.bmm` | `plmc_cross_matvec_f32` (the values) | pair derivatives / s, fused | faster route |",
         "|---|---|---|---|---|---|---|---|---|"]
for ns in (64, 2048):
    Xs = (2 * torch.rand(ns, d, generator=g) - 1).to(dev)
    for r in (1, 8):
        V = torch.randn(q, n, r, generator=g).to(dev)
        G = torch.randn(q, ns, r, generator=g).to(dev)

        def fused():
            return _engine.cross_matvec_dx("matern52", Xs, X, ell, None, V, G)

        def bmm():
            return torch.bmm(V, G.transpose(1, 2))                      # (q, n, n*)

        def composed():
            return _engine.posterior_dx("matern52", X, Xs, ell, None, alpha, bmm())[1]

        def values():
            return _engine.cross_matvec("matern52", Xs, X, ell, None, V)

        tf, tc, tb, tv = timed([fused, composed, bmm, values], a.reps)
        want = -0.5 * composed()
        err = float((fused() - want).abs().max() / want.abs().max())
        lines.append("| %d | %d | %d | %.3f ms | %.3f ms (%d) | %.3f ms | %.3f ms | %.3g | %s |"
                     % (ns, r, L.plmc_cross_matvec_dx_splits(n, ns, q), tf, tc, _engine.posterior_dx_splits(n, ns, q), tb, tv,
                        q * n * ns / (tf * 1e-3), "fused" if tf <= tc else "composed"))
        lines.append("| | | (largest difference of the two routes, relative to the largest element: %.2e) | | | | | | |" % err)
text = "\n".join(lines) + "\n"
print(text)
if a.md:
    with open(a.md, "w") as f:
        f.write(text)
