"""Time of the component-table kernel VJP (`plmc_kernel_vjp_add_f32`) at the pull-back shapes of BASELINE config 4 (m = 2000 inducing
points, n = 3000, q = 8, d = 8) with decomp=[[0,1,2,3],[4,5,6,7]], for the K_ZZ (m x m) and the K_ZX (m x n) call, beside the plain
`plmc_kernel_vjp_f32` at the same shapes IN THE SAME RUN (the yardstick: both read G once).  HIP events around each launch, warm-up, the
median of repeated launches, the two kernels alternating.  Needs the MI355X; prints the table and, with --out FILE, writes it there.
    python tools/vjp_add_time.py --out profiles/vjp_add_time.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "projected-lmc_amd")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from projectedlmc import _hip
    assert torch.cuda.is_available(), "vjp_add_time.py needs the GPU"
    dev, dt = torch.device("cuda:0"), torch.float32
    L = _hip.lib()
    d, groups = 8, [[0, 1, 2, 3], [4, 5, 6, 7]]
    g = torch.Generator().manual_seed(0)
    Z = (2 * torch.rand(a.m, d, generator=g) - 1).to(dev)
    X = (2 * torch.rand(a.n, d, generator=g) - 1).to(dev)
    ell = (1.0 + torch.rand(a.q, d, generator=g)).to(dev)
    table = torch.full((a.q, len(groups), d), float("inf"))
    for i, idx in enumerate(groups):
        table[:, i, idx] = ell[:, idx].cpu()
    table = table.to(dev)
    osc, osc_t = torch.ones(a.q, device=dev), torch.ones(a.q, len(groups), device=dev)
    st = _hip.stream_ptr(dev)
    kind = _hip.KIND["matern52"]
    lines = ["kernel VJP, fp32, matern52, q = %d, d = %d, decomp = %s; median of %d launches after %d warm-up launches (HIP events)"
             % (a.q, d, groups, a.reps, a.warmup),
             "%-6s %6s %6s %12s %12s %8s %14s %14s" % ("call", "n1", "n2", "plain ms", "table ms", "ratio", "plain GB/s", "table GB/s")]
    for name, X2 in (("K_ZZ", Z), ("K_ZX", X)):
        n1, n2 = a.m, X2.shape[0]
        G = torch.randn(a.q, n1, n2, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        gX = torch.empty(a.q, n1, d, dtype=torch.float64, device=dev)
        gE = torch.empty(a.q, n1, len(groups), d, dtype=torch.float64, device=dev)
        gO = torch.empty(a.q, n1, len(groups), dtype=torch.float64, device=dev)
        out = (_hip.ptr(G), n2, n1 * n2, _hip.ptr(gX), _hip.ptr(gE), _hip.ptr(gO), a.q, st)

        def plain():
            L.call("plmc_kernel_vjp", dt, kind, _hip.ptr(Z), n1, _hip.ptr(X2), n2, d, _hip.ptr(ell), _hip.ptr(osc), *out)

        def tab():
            L.call("plmc_kernel_vjp_add", dt, kind, _hip.ptr(Z), n1, _hip.ptr(X2), n2, d, len(groups), _hip.ptr(table), _hip.ptr(osc_t), *out)

        times = {plain: [], tab: []}
        for it in range(a.warmup + a.reps):
            for fn in (plain, tab):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[fn].append(e0.elapsed_time(e1))
        tp, tt = statistics.median(times[plain]), statistics.median(times[tab])
        nbytes = a.q * n1 * n2 * 4.0                                # G, read once by both
        lines.append("%-6s %6d %6d %12.4f %12.4f %8.3f %14.1f %14.1f" % (name, n1, n2, tp, tt, tt / tp, nbytes / tp / 1e6, nbytes / tt / 1e6))
        lines.append("       spread (min / max ms): plain %.4f / %.4f, table %.4f / %.4f"
                     % (min(times[plain]), max(times[plain]), min(times[tab]), max(times[tab])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
