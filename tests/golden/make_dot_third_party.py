"""Generates tests/golden/dot_third_party_v1.json -- run from the repo root:  python tests/golden/make_dot_third_party.py

INDEPENDENT cross-check of the dense reference of the dot-product kernels (tests/_dot_dense.py), in the manner of
make_sum_third_party.py: scikit-learn's GaussianProcessRegressor with
    ConstantKernel * Exponentiation(DotProduct(sigma_0), P) + WhiteKernel        (P = 1: ConstantKernel * DotProduct + WhiteKernel)
on n = 40 uniform points of [-1, 1]^3.  scikit-learn's DotProduct is sigma_0^2 + x . x', so the offset of this project is c = sigma_0^2
(the test applies the chain rule d / d log sigma_0 = 2 c d / d c), and the variances v enter through pre-scaled inputs sqrt(v) x.  One
case per power, the linear one with sigma_0 at scikit-learn's lower bound of the value (1e-5: c = 1e-10, the linear kernel to 1e-10).
Stored per case: the inputs, the natural parameters, the upper triangle of the kernel matrix K (noise included) row by row, the log
marginal likelihood and its gradient in scikit-learn's log-parameters with their names.  Only numbers are stored; nothing of the library
travels."""
import json
import os

import numpy as np
import sklearn
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, DotProduct, Exponentiation, WhiteKernel

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dot_third_party_v1.json")
CASES = [dict(power=1, sigma_0=1.0e-5, os=0.7, noise=0.2, v=[0.5, 1.3, 2.0]),
         dict(power=1, sigma_0=0.8, os=1.4, noise=0.1, v=[1.0, 1.0, 1.0]),
         dict(power=2, sigma_0=0.9, os=0.6, noise=0.3, v=[1.0, 1.0, 1.0]),
         dict(power=3, sigma_0=1.2, os=0.25, noise=0.15, v=[0.7, 1.1, 0.4])]


def main():
    rng = np.random.RandomState(0)
    n, d = 40, 3
    out = {"generator": "tests/golden/make_dot_third_party.py", "scikit_learn": sklearn.__version__, "numpy": np.__version__, "cases": []}
    for P in CASES:
        X = rng.uniform(-1.0, 1.0, (n, d))
        Xv = X * np.sqrt(np.asarray(P["v"]))[None, :]
        dot = DotProduct(sigma_0=P["sigma_0"], sigma_0_bounds=(1e-6, 1e5))
        core = dot if P["power"] == 1 else Exponentiation(dot, P["power"])
        kernel = ConstantKernel(P["os"]) * core + WhiteKernel(P["noise"])
        K = kernel(Xv)
        y = np.linalg.cholesky(K) @ rng.normal(size=n)
        gpr = GaussianProcessRegressor(kernel=kernel, optimizer=None, alpha=0.0).fit(Xv, y)
        theta = gpr.kernel_.theta
        names = [h.name for h in gpr.kernel_.hyperparameters]
        lml, glog = gpr.log_marginal_likelihood(theta, eval_gradient=True)
        out["cases"].append({"params": P, "X": X.tolist(), "y": y.tolist(), "K_upper": K[np.triu_indices(n)].tolist(),
                             "cond": float(np.linalg.cond(K)), "theta_names": names, "theta": theta.tolist(),
                             "log_marginal_likelihood": float(lml), "grad_log_theta": glog.tolist()})
        print("P = %d: lml %.6f, cond %.3g, %s" % (P["power"], lml, out["cases"][-1]["cond"], names))
    json.dump(out, open(OUT, "w"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
