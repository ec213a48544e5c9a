"""Time of plmc_cross_matvec_f32 at the metric shape (n = 8192, q = 8, d = 8, Matern-5/2, fp32), r = 1 and r = 8, n* in {2048, 131072},
beside the yardstick plmc_assemble_cross_f32 at the same shape -- the same evaluations, written out -- and a matvec over its output
(torch.bmm), and of a mean-only prediction (settings.skip_posterior_variances) beside the cached default prediction at n* = 2048.
Device events around every call, median of --reps calls after 3 warm-up calls, the kinds alternating call by call in one process.
`python tools/cross_matvec_time.py [--md profiles/cross_matvec_time.md] [--n 8192] [--reps 20]`"""
import argparse
import os
import statistics
import sys
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--big", type=int, default=131072)
ap.add_argument("--md", default=None)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
import projectedlmc as plmc  # noqa: E402
from projectedlmc import _engine, _hip, settings  # noqa: E402

assert torch.cuda.is_available(), "tools/cross_matvec_time.py measures on the GPU only"
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
V = torch.randn(q, n, 8, generator=g).to(dev)
alpha = V[:, :, 0].contiguous()
lines = ["| n* | ranges (`plmc_cross_matvec_splits`) | `plmc_cross_matvec_f32` r = 1 | r = 8 | `plmc_assemble_cross_f32` (writes q n n* values) | + `torch.bmm` "
         "over its output, r = 1 | r = 8 | evaluations / s, r = 1 |", "|---|---|---|---|---|---|---|---|"]
for ns in (2048, a.big):
    Xs = (2 * torch.rand(ns, d, generator=g) - 1).to(dev)
    K = torch.empty(q, ns, n, dtype=dt, device=dev)                     # K(X*, X): rows = test points (plmc_assemble_cross with X1 = X*)

    def cm1():
        _engine.cross_matvec("matern52", Xs, X, ell, None, alpha)

    def cm8():
        _engine.cross_matvec("matern52", Xs, X, ell, None, V)

    def cross():
        _engine._kernel_call(_hip.lib(), "plmc_assemble_cross", dt, (_hip.KIND["matern52"], _hip.ptr(Xs), ns, _hip.ptr(X), n, d), ell,
                             (None, _hip.ptr(K), n, ns * n, 0, ns, q, _hip.stream_ptr(dev)))

    def mv1():
        torch.bmm(K, alpha.unsqueeze(-1))

    def mv8():
        torch.bmm(K, V)

    t1, t8, tc, tm1, tm8 = timed([cm1, cm8, cross, mv1, mv8], a.reps if ns <= 4096 else max(5, a.reps // 4))
    cross()
    ref = torch.bmm(K[:, :2048].double(), alpha.double().unsqueeze(-1)).squeeze(-1)          # (the first 2048 test points)
    err = float((_engine.cross_matvec("matern52", Xs, X, ell, None, alpha)[:, :2048].double() - ref).abs().max() / ref.abs().max())
    lines.append("| %d | %d | %.3f ms | %.3f ms | %.3f ms | %.3f ms | %.3f ms | %.3g |"
                 % (ns, _engine.cross_matvec_splits(n, ns, q), t1, t8, tc, tc + tm1, tc + tm8, q * n * ns / (t1 * 1e-3)))
    lines.append("| | | (largest difference from the dense product, relative to its largest element: %.2e) | | | | | |" % err)
    del K
    torch.cuda.empty_cache()

# ---- the prediction: cached default route against the mean-only route, n* = 2048, the projected model of bench.py's shape
p, ns = 16, 2048
Y = torch.randn(n, p, generator=g)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    m = plmc.ProjectedGPModel(X.cpu(), Y, p, q, mean_type=plmc.ZeroMean, kernel_type=plmc.MaternKernel, init_lmc_coeffs=True).to(dev).eval()
Xs = (2 * torch.rand(ns, d, generator=g) - 1).to(dev)


def full():
    with torch.no_grad():
        return m(Xs).mean


def only():
    with torch.no_grad(), settings.skip_posterior_variances():
        return m(Xs).mean


with settings.prediction_cache("eager"):
    full(), only()
    tf, to = timed([full, only], a.reps)
    diff = float((full() - only()).abs().max())
pred = ["| what (n = %d, n* = %d, q = %d, p = %d, fp32, cache hit) | ms per call |" % (n, ns, q, p), "|---|---|",
        "| default prediction: cross-covariance columns, forward substitution, moments | %.3f |" % tf,
        "| `settings.skip_posterior_variances()`: K(x*, X) alpha from the cached alpha | %.3f |" % to,
        "| largest difference of the two means | %.2e |" % diff]
text = "\n".join(lines) + "\n\n" + "\n".join(pred) + "\n"
print(text)
if a.md:
    with open(a.md, "w") as f:
        f.write(text)
