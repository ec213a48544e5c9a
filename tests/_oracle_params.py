"""The oracle's parameter dict of a ProjectedGPModel, for tests that compare the model with oracle/projected.py on the host."""
import math


def oracle_dict(model):
    """The oracle's parameter dict (oracle/projected.py) WITHOUT kernel keys, from the state dict, as oracle/bridge.py reads it
    (bulk H, or the parametrised Q_plus . R of bulk=False); the kernel's entries of the state dict; and the map model parameter
    name -> dict key."""
    lb = model.likelihood.noise_covar.raw_noise_constraint.lower_bound
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lmc = model.lmc_coefficients
    P = dict(n_tasks=model.n_tasks, n_latents=model.n_latents, mode=lmc.mode, BDN=not hasattr(model, "M"), eps=model.eps,
             scalar_B=model.scalar_B, diagonal_B=model.diagonal_B, noise_lb=lb, noise_thresh=math.log(lb), bulk=lmc.bulk,
             raw_noise=sd["likelihood.noise_covar.raw_noise"], B_tilde_inv_chol_raw=sd["parametrizations.B_tilde_inv_chol.original"])
    names = {"likelihood.noise_covar.raw_noise": "raw_noise", "parametrizations.B_tilde_inv_chol.original": "B_tilde_inv_chol_raw"}
    if lmc.bulk:
        P["H"] = sd["lmc_coefficients.H"]
        names["lmc_coefficients.H"] = "H"
    else:
        P["Q_plus_original"] = sd["lmc_coefficients.parametrizations.Q_plus.original"]
        P["Q_plus_base"] = sd.get("lmc_coefficients.parametrizations.Q_plus.0.base")
        P["ortho_param"] = lmc.parametrizations.Q_plus[0].orthogonal_map.name
        P["R_original"] = sd["lmc_coefficients.parametrizations.R.original"]
        P["diagonal_R"] = type(lmc.parametrizations.R[0]).__name__ == "PositiveDiagonalParam"
        names["lmc_coefficients.parametrizations.Q_plus.original"] = "Q_plus_original"
        names["lmc_coefficients.parametrizations.R.original"] = "R_original"
    kern = {k: v for k, v in sd.items() if k.startswith("covar_module.")}
    return P, kern, names
