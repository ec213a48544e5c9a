"""Timing of get_fantasy_model against the refit it replaces: ExactGPModel with q = 8 batch tasks, n = 8192, d = 8,
n* = 2048, fp32, m = 1, 16, 128 new observations.  In one process, per m (median of REPS):
    fantasy     base.get_fantasy_model(X_new, y_new) + the copy's first prediction (a cache hit on the extended factor)
    refit eager set_train_data([X; X_new]) on a copy + its first prediction under prediction_cache("eager"): the sweep with the inverse
                factor and the kept planes -- what leaves the refit model in the state the fantasy model is in (a cache for later calls)
    refit lazy  the same under the default prediction_cache("lazy"): the plain augmented sweep, no cache kept
    python tools/fantasy_time.py [n] [n_star] -> one JSON line per m."""
import copy, json, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]
import torch
import projectedlmc as plmc
from projectedlmc import settings

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
d, q, REPS, MS = 8, 8, 3, (1, 16, 128)
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
X = 2 * torch.rand(n + max(MS), d, generator=g) - 1
Y = torch.randn(n + max(MS), q, generator=g)
Xs = (2 * torch.rand(ns, d, generator=g) - 1).to(dev)
torch.manual_seed(0)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    base = plmc.ExactGPModel(X[:n], Y[:n], plmc.GaussianLikelihood(batch_shape=torch.Size([q])), n_tasks=q, kernel_type=plmc.MaternKernel,
                             mean_type=plmc.ZeroMean)
base = base.to(dev).eval()
X, Y = X.to(dev), Y.to(dev)


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def predict(model):
    with torch.no_grad():
        out = model(Xs)
        return out.mean, out.variance


def fantasy(m):
    t_ext, fant = clock(lambda: base.get_fantasy_model(X[n:n + m], Y[n:n + m]))
    t_pred, (mean, var) = clock(lambda: predict(fant))
    c = fant._prediction_cache()
    assert (c.hits, c.misses) == (1, 0), (c.hits, c.misses)
    return t_ext, t_pred, mean, var


def refit(m, mode):
    ref = copy.deepcopy(base)
    with settings.prediction_cache(mode):
        def run():
            ref.set_train_data(X[:n + m], Y[:n + m])
            return predict(ref)
        t, (mean, var) = clock(run)
    return t, mean, var


med = lambda v: sorted(v)[len(v) // 2]
with settings.prediction_cache("eager"):
    t_base, _ = clock(lambda: predict(base))               # builds the base cache (sweep with the inverse factor and the kept planes)
    fantasy(1); refit(1, "eager"); refit(1, "lazy")        # warm-up: code objects, allocator
    for m in MS:
        f = [fantasy(m) for _ in range(REPS)]
        e = [refit(m, "eager") for _ in range(REPS)]
        l = [refit(m, "lazy") for _ in range(REPS)]
        dm = float((f[0][2] - e[0][1]).abs().max() / e[0][1].abs().max())
        dv = float((f[0][3] - e[0][2]).abs().max() / e[0][2].abs().max())
        print(json.dumps({"n": n, "q": q, "d": d, "n_star": ns, "m": m, "dtype": "f32", "base_cache_build_call_ms": t_base,
                          "fantasy_extend_ms": med([x[0] for x in f]), "fantasy_first_prediction_ms": med([x[1] for x in f]),
                          "fantasy_total_ms": med([x[0] + x[1] for x in f]), "refit_eager_ms": med([x[0] for x in e]),
                          "refit_lazy_ms": med([x[0] for x in l]), "mean_rel_diff_to_refit": dm, "var_rel_diff_to_refit": dv}), flush=True)
