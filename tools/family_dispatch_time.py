"""Host time of the Python family dispatch: _engine._kernel_call("plmc_assemble", ...) on a warm table per covariance family, on CPU
tensors with a stand-in for the library that only records (no GPU, no library call).  Two checkouts are compared, alternated:

    python tools/family_dispatch_time.py PARENT/projected-lmc_amd RESULT/projected-lmc_amd

5 repeats of 20 000 calls per family and side, each repeat in a fresh process; prints one markdown table
(profiles/family_dispatch_host_time.md).
"""
import json
import statistics
import subprocess
import sys
import time

N, REPEATS = 20000, 5
FAMILIES = [("plain", "matern52", (2, 3)), ("add", "matern52", (2, 2, 3)), ("sm", "sm", (2, 2, 4, 3)), ("periodic", "periodic", (2, 2, 3)),
            ("rq", "rq", (2, 4)), ("locally_periodic", "locally_periodic", (2, 3, 3)), ("sum", "sum(rbf,periodic)", (2, 2, 10)),
            ("linear", "linear", (2, 4))]


class Recorder:
    def call(self, name, dt, *args):
        self.last = args


def child(pkg):
    sys.path.insert(0, pkg)
    import torch
    from projectedlmc import _engine
    out, L, call = {}, Recorder(), _engine._kernel_call
    for label, kind, shape in FAMILIES:
        ell = torch.ones(*shape, dtype=torch.float64)
        head = (_engine.kind_code(kind), None, 100, 3)
        tail = (None, None, None, 128, 128 * 128, 2, None)
        for _ in range(200):                # the table is split here
            call(L, "plmc_assemble", torch.float64, head, ell, tail)
        t0 = time.perf_counter()
        for _ in range(N):
            call(L, "plmc_assemble", torch.float64, head, ell, tail)
        out[label] = (time.perf_counter() - t0) / N * 1e6
    print(json.dumps(out))


def main(parent, result):
    runs = {"parent": [], "result": []}
    for _ in range(REPEATS):
        for name, pkg in (("parent", parent), ("result", result)):
            o = subprocess.run([sys.executable, __file__, "--child", pkg], capture_output=True, text=True, check=True).stdout
            runs[name].append(json.loads(o.strip().splitlines()[-1]))
    print("| family | parent min | parent median | parent max | result min | result median | result max | result median in parent's range |")
    print("|---|---|---|---|---|---|---|---|")
    for label, _, _ in FAMILIES:
        p, r = [x[label] for x in runs["parent"]], [x[label] for x in runs["result"]]
        med = statistics.median(r)
        verdict = "yes" if min(p) <= med <= max(p) else ("below" if med < min(p) else "above")
        print("| %s | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %s |" % (label, min(p), statistics.median(p), max(p), min(r), med, max(r), verdict))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main(sys.argv[1], sys.argv[2])
