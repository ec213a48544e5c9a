"""Generates tests/golden/sum_third_party_v1.json -- run from the repo root:  python tests/golden/make_sum_third_party.py

INDEPENDENT cross-check of the dense reference of a sum of kernel families (tests/_sum_dense.py), in the manner of
make_third_party.py: scikit-learn's GaussianProcessRegressor with
    ConstantKernel * RBF + ConstantKernel * ExpSineSquared * RBF + ConstantKernel * RationalQuadratic + WhiteKernel
on n = 300 sorted uniform points of [0, 10], d = 1 -- trend + a periodicity that drifts + medium-term irregularity.  Stored: the inputs,
the natural parameters, the kernel matrix K (noise included) at every tenth point -- the upper triangle of K[::10, ::10], row by row: the
fixture stays small, and every element of K enters the next two --, the log marginal likelihood and its gradient in scikit-learn's
log-parameters with their names.  scikit-learn's ExpSineSquared is exp(-2 sin^2(pi tau / p) / l^2): its length scale enters
squared, so the periodic lengthscale of this project is l^2 (the test applies the chain rule).  Only numbers are stored; nothing of the
library travels."""
import json
import os

import numpy as np
import sklearn
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, ExpSineSquared, RationalQuadratic, WhiteKernel

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sum_third_party_v1.json")
PARAMS = dict(os_rbf=0.6, ell_rbf=2.5, os_lper=0.5, ell_ess=1.1, period=1.7, ell_drift=4.0, os_rq=0.2, alpha=1.5, ell_rq=0.6, noise=0.08)


def main():
    P = PARAMS
    rng = np.random.RandomState(0)
    n = 300
    X = np.sort(rng.uniform(0.0, 10.0, n))[:, None]
    kernel = (ConstantKernel(P["os_rbf"]) * RBF(P["ell_rbf"])
              + ConstantKernel(P["os_lper"]) * ExpSineSquared(length_scale=P["ell_ess"], periodicity=P["period"]) * RBF(P["ell_drift"])
              + ConstantKernel(P["os_rq"]) * RationalQuadratic(length_scale=P["ell_rq"], alpha=P["alpha"]) + WhiteKernel(P["noise"]))
    K = kernel(X)
    y = np.linalg.cholesky(K) @ rng.normal(size=n)
    gpr = GaussianProcessRegressor(kernel=kernel, optimizer=None, alpha=0.0).fit(X, y)
    theta = gpr.kernel_.theta
    names = [h.name for h in gpr.kernel_.hyperparameters]
    lml, glog = gpr.log_marginal_likelihood(theta, eval_gradient=True)
    STRIDE = 10
    Ks = K[::STRIDE, ::STRIDE]
    iu = np.triu_indices(Ks.shape[0])
    out = {"generator": "tests/golden/make_sum_third_party.py", "scikit_learn": sklearn.__version__, "numpy": np.__version__,
           "params": P, "X": X[:, 0].tolist(), "y": y.tolist(), "K_stride": STRIDE, "K_upper": Ks[iu].tolist(), "cond": float(np.linalg.cond(K)),
           "theta_names": names, "theta": theta.tolist(), "log_marginal_likelihood": float(lml), "grad_log_theta": glog.tolist()}
    json.dump(out, open(OUT, "w"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; lml %.6f, cond %.3g" % (lml, out["cond"]))
    print(names)


if __name__ == "__main__":
    main()
