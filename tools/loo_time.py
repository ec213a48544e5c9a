"""Time of one leave-one-out step (value + backward) beside one MLL step (dev aid): python tools/loo_time.py [n] [q].
fp32, matern52, d = 8; device events around `reps` steps after warm-up."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]
import torch
from projectedlmc import _engine

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
q = int(sys.argv[2]) if len(sys.argv) > 2 else 8
d, warm, reps = 8, 3, 5
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
X = (2 * torch.rand(n, d, generator=g) - 1).to(dev)
y = torch.randn(q, n, generator=g).to(dev)
ell = torch.full((q, d), 0.7, device=dev, requires_grad=True)
noise = torch.full((q,), 0.7, device=dev, requires_grad=True)


def step(fn):
    ell.grad = noise.grad = None
    fn("matern52", X, ell, None, noise, y).sum().backward()


for name, fn in (("mll", _engine.exact_latent_log_prob), ("loo", _engine.exact_loo_log_prob)):
    for _ in range(warm):
        step(fn)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step(fn)
    e1.record()
    torch.cuda.synchronize()
    print("%s step n=%d q=%d fp32: %.2f ms (value + backward, mean of %d)" % (name, n, q, e0.elapsed_time(e1) / reps, reps))
    _engine.free_workspaces()
