"""Time of a prediction that is differentiable in hyper-parameters, noise and targets (settings.posterior_hyper_grad) at the metric shape:
ExactGPModel, q = 8 independent tasks, n = 8192, d = 8, fp32 Matern-5/2, n* in {16, 2048}, a loss of the mean alone
(predictive_variance_grad(False), r = 2) and of mean and variance (r = n* + 2), on a cache hit.  Per case: the weighted kernel-gradient
sum alone (plmc_weighted_grad_f32 on operands of that shape), the whole forward + backward with the setting on, and the same prediction
with the setting off (no graph).  A tree without the setting (the parent commit), or --off-only, reports the last column only: run that
way in both trees, alternating, it is the off-path comparison; --dump FILE keeps that prediction's mean and variance for a bit compare.
Device events around every call, median of --reps calls after 3 warm-up calls, the variants alternating call by call in one process.
`python tools/posterior_hyper_grad_time.py [--md profiles/posterior_hyper_grad_time.md] [--n 8192] [--reps 10] [--off-only] [--dump FILE]`"""
import argparse
import os
import statistics
import sys
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--md", default=None)
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--dump", default=None)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
import projectedlmc as plmc  # noqa: E402
from projectedlmc import _engine, settings  # noqa: E402

assert torch.cuda.is_available(), "tools/posterior_hyper_grad_time.py measures on the GPU only"
dev = torch.device("cuda:0")
dt = torch.float32
n, q, d = a.n, 8, 8
WARM = 3
HAVE = hasattr(settings, "posterior_hyper_grad") and not a.off_only
kept = {}


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
X = 2 * torch.rand(n, d, generator=g) - 1
Y = torch.stack([torch.sin(2.0 * X[:, 0] + k) * torch.cos(X[:, 1] - X[:, 2]) + 0.1 * torch.randn(n, generator=g) for k in range(q)])
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    m = plmc.ExactGPModel(X, Y, plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q, kernel_type=plmc.MaternKernel)
m.likelihood.noise = 0.05
m = m.to(dev).eval()
lines = ["| n* | loss | r_pad | N_pad | `plmc_weighted_grad_f32` alone | TFLOP/s (q N_pad^2 r_pad multiply-adds, upper tiles) | forward + backward, setting on "
         "| same prediction, setting off (no graph) | mean / variance bit-equal on / off |", "|---|---|---|---|---|---|---|---|---|"]
with settings.prediction_cache("eager"):
    for ns in (16, 2048):
        Xs = (2 * torch.rand(ns, d, generator=g) - 1).to(dev)
        wm, wv = torch.randn(q, ns, generator=g).to(dev), torch.randn(q, ns, generator=g).to(dev)

        def off():
            with torch.no_grad():
                out = m(Xs)
                return out.mean, out.variance

        kept[ns] = tuple(t.cpu() for t in off())
        if not HAVE:
            lines.append("| %d | - | - | - | - | - | - | %.3f ms | - |" % (ns, timed([off], a.reps)[0]))
            continue
        for variance in (False, True):
            def on():
                for p_ in m.parameters():
                    p_.grad = None
                with settings.posterior_hyper_grad(True), settings.predictive_variance_grad(variance):
                    out = m(Xs)
                    loss = (wm * out.mean).sum() + ((wv * out.variance).sum() if variance else 0.0)
                    loss.backward()
                return out.mean.detach(), out.variance.detach()

            r = ns + 2 if variance else 2
            r_pad, N = -(-r // 16) * 16, n + ns
            N_pad = -(-N // 128) * 128
            At = torch.randn(q, r_pad, N_pad, generator=g).to(dev)
            At[:, r:] = 0
            At[:, :, N:] = 0
            Z = torch.cat([X.to(dev), Xs])
            ell = (0.6 + 0.8 * torch.rand(q, d, generator=g)).to(dev)

            def kern():
                _engine.weighted_grad("matern52", Z, ell, None, At, At, N)

            tk, ton, toff = timed([kern, on, off], a.reps)
            same = all(torch.equal(x_, y_) for x_, y_ in zip(on(), off()))
            lines.append("| %d | %s | %d | %d | %.3f ms | %.1f | %.3f ms | %.3f ms | %s |"
                         % (ns, "mean and variance" if variance else "mean only", r_pad, N_pad, tk,
                            2.0 * q * (N_pad * (N_pad + 128) / 2) * r_pad / (tk * 1e-3) / 1e12, ton, toff, same))
            del At
            torch.cuda.empty_cache()
if a.dump:
    torch.save(kept, a.dump)
text = "\n".join(lines) + "\n"
print(text)
if a.md:
    with open(a.md, "w") as f:
        f.write(text)
