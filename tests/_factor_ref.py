"""LAPACK-style test of the blocked factorisation (csrc/potrf.hip): inputs, buffer layout, fp64 reference, measures, thresholds.

Shared by tests/test_factor_ref_host.py (CPU: the reference alone passes, seeded mutations fail) and tests/test_gpu_factor.py
(the sweep itself).  CPU only: nothing here imports the library or touches a GPU; the residual products run wherever the
tensors they are given live.

Inputs.  Every matrix is built in fp64 from a seeded generator and ROUNDED to the element type; the reference factorises the
rounded matrix, so the rounding of the input is not counted as error.  All families have kappa_2(K) <= 100 (asserted from
eigvalsh) and come with a true lower bound of the smallest eigenvalue (asserted too), as the fp16 split needs.

Measures (u = 2^-24 / 2^-53 for the element type; per latent; residuals and tiles over the whole n_pad x n_pad matrices padded
with the identity, the NORMS of K, U, W over their leading n x n parts -- the padding decouples and is exact, and its ones would
otherwise swamp the norm of a matrix scaled by 1e-3; kappa_2 likewise is that of K itself):
    rho_U = |U^T U - K|_F / (n_pad u |K|_F)
    rho_W = |W U^T - I|_F / (n_pad u |U|_F |W|_F)
    rho_Z = max over columns |U^T z - b|_2 / (n_pad u |U|_F |z|_2)
    e_U   = max over 128 x 128 tiles |U - U_ref|_F(tile) / |U_ref|_F,  e_W, e_Z likewise (the tile is named)
U_ref, W_ref = U_ref^-T, Z_ref: torch.linalg.cholesky / solve_triangular in fp64 on the CPU.

Thresholds, none tuned on the code under test.  "reference measure" = the same measure of the CPU LAPACK factorisation of the
same rounded matrix in the same element type (`lapack_factor`).
  * fp64, and fp32 on the fp32 matrix instructions:  measure <= (1 + sqrt kappa_2(K)) max(reference measure, floor).
    sqrt kappa: the group panel multiplies by the explicitly inverted group triangle, whose error bound carries
    kappa(U_gg) <= sqrt kappa_2(K) over substitution.  Floor of the rho measures: 1 (one rho unit: the rounding of the fp64
    evaluation of the residual itself).  Floor of the e measures: the accuracy of the fp64 REFERENCE, kappa_2(K)^(3/2) n_pad 2^-53
    -- a backward error of one fp64 rho unit through the first-order perturbation bound of the Cholesky factor
    (|dU|_F / |U|_2 <= kappa_2(K) eps / sqrt 2, Sun 1991) and one more kappa(U) = sqrt kappa_2(K) for W = U^-T and Z = U^-T B;
    for fp64 the LAPACK factorisation IS the reference (its e is 0) and only this floor is left.
  * split schemes:  measure_split < 2 measure_plain + 2e-6 on RELATIVE quantities (e as it is, rho n_pad u), plain = the same
    call under PLMC_SPLIT=0 -- the rule of test_split_engines_against_fp32_mfma_path -- and rho_U inside the a-priori bound
    of DESIGN.md 3.4 (`split_apriori_rho_u`).
"""
import math

import torch

NB = 128
UNIT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
KAPPA_MAX = 100.0
GRADED_SCALES = (1e-3, 1.0, 1e3)


def pad(n):
    return (n + NB - 1) // NB * NB


class HostWorkspace:
    """The factor buffer of projectedlmc._engine.Workspace (same geometry, include/plmc.h) as host tensors: what a sweep
    would be handed, for the checks that run without the library."""

    def __init__(self, n, q, naug, dtype, with_inverse=True):
        self.n, self.q, self.naug, self.dtype, self.with_inverse = n, q, naug, dtype, bool(with_inverse)
        self.NB, self.n_pad = NB, pad(n)
        self.naug_pad = pad(naug) if naug > 0 else 0
        self.wcol0 = self.n_pad + self.naug_pad
        self.lda = self.wcol0 + (self.n_pad if with_inverse else 0)
        if (self.lda // NB) % 2 == 0:
            self.lda += NB
        self.strideA = self.n_pad * self.lda
        self.m = self.n_pad // NB
        self.A = torch.empty(q, self.n_pad, self.lda, dtype=dtype)
        self.logdet = torch.empty(q, dtype=torch.float64)
        self.info = torch.empty(q, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ matrix families
def _round(K, dtype):
    """fp64 values of the matrix rounded to `dtype`, symmetric"""
    K = K.to(dtype).double()
    return 0.5 * (K + K.transpose(-1, -2))


def _wishart64(n, q, gen, s2):
    k = max(n // 2, 1)
    B = torch.randn(q, n, k, generator=gen, dtype=torch.float64)
    s2 = torch.as_tensor(s2, dtype=torch.float64).reshape(-1, 1, 1)
    return B @ B.transpose(1, 2) / k + s2 * torch.eye(n, dtype=torch.float64), s2.reshape(-1).expand(q).clone()


class Case:
    """q matrices of one family at one (n, dtype), with everything the checks need that depends on them alone."""

    def __init__(self, family, n, q, dtype, seed=0):
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * n + {"wishart": 1, "graded": 2, "kernel": 3}[family])
        self.family, self.n, self.q, self.dtype, self.n_pad, self.gen = family, n, q, dtype, pad(n), gen
        self.params = None
        if family == "wishart":
            K, lo = _wishart64(n, q, gen, [0.1 * 2 ** i for i in range(q)])
        elif family == "graded":
            assert q == len(GRADED_SCALES)
            C, lo = _wishart64(n, q, gen, 0.1)
            D = torch.tensor(GRADED_SCALES, dtype=torch.float64)
            K, lo = D.reshape(-1, 1, 1) * C, D * lo                      # D^(1/2) C D^(1/2) with one scalar D per latent
        elif family == "kernel":
            from oracle import gp_math as gm
            d = 3
            X = 2 * torch.rand(n, d, generator=gen, dtype=torch.float64) - 1
            ell = 0.10 + 0.06 * torch.rand(q, d, generator=gen, dtype=torch.float64)
            osc = 0.8 + 0.5 * torch.rand(q, generator=gen, dtype=torch.float64)
            noise = 0.5 + 0.5 * torch.rand(q, generator=gen, dtype=torch.float64)
            # the parameters are rounded first: the library's assembler is given exactly these numbers
            X, ell, osc, noise = (t.to(dtype).double() for t in (X, ell, osc, noise))
            K = gm.kernel_matrix("matern", X, X, ell, osc, 2.5) + noise.reshape(-1, 1, 1) * torch.eye(n, dtype=torch.float64)
            lo = noise.clone()                                           # K is positive semi-definite
            self.params = dict(X=X, ell=ell, oscale=osc, noise=noise, d=d)
        else:
            raise ValueError(family)
        self.K = _round(K, dtype)
        ev = torch.linalg.eigvalsh(self.K)
        self.eig_min, self.eig_max = ev[:, 0].clone(), ev[:, -1].clone()
        self.kappa = self.eig_max / self.eig_min                         # lambda_max / lambda_min in fp64
        self.eig_lo = 0.9 * lo                                           # the rounding of K moves eigenvalues by << 0.1 lo
        assert bool((self.kappa <= KAPPA_MAX).all()), (family, n, self.kappa.tolist())
        assert bool((self.eig_lo <= self.eig_min).all()) and bool((self.eig_lo > 0).all()), (self.eig_lo.tolist(), self.eig_min.tolist())
        self._ref = None
        self._lapack = None

    def K_pad(self, K=None):
        K = self.K if K is None else K
        Kp = torch.eye(self.n_pad, dtype=torch.float64).repeat(self.q, 1, 1)
        Kp[:, :self.n, :self.n] = K
        return Kp

    def rhs(self, naug, col_scales=None, seed=0):
        """(q, naug, n) right-hand sides rounded to the element type; col_scales: one factor per column"""
        g = torch.Generator().manual_seed(4241 * self.n + naug + 104729 * seed)
        b = torch.randn(self.q, naug, self.n, generator=g, dtype=torch.float64)
        if col_scales is not None:
            b = b * torch.as_tensor(col_scales, dtype=torch.float64).reshape(1, naug, 1)
        return b.to(self.dtype).double()

    def rhs_pad(self, rhs):
        """(q, n_pad, naug): columns, padded rows zero"""
        B = torch.zeros(self.q, self.n_pad, rhs.shape[1], dtype=torch.float64)
        B[:, :self.n] = rhs.transpose(1, 2)
        return B

    # fp64 reference: L L^T = K_pad; U_ref = L^T, W_ref = U_ref^-T = L^-1 (computed once per case)
    def ref(self):
        if self._ref is None:
            L = torch.linalg.cholesky(self.K_pad())
            W = torch.linalg.solve_triangular(L, torch.eye(self.n_pad, dtype=torch.float64).expand(self.q, -1, -1), upper=False)
            self._ref = dict(U=L.transpose(1, 2).contiguous(), W=torch.tril(W), L=L,
                             logdet=2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(-1))
        return self._ref

    def z_ref(self, rhs):
        return torch.linalg.solve_triangular(self.ref()["L"], self.rhs_pad(rhs), upper=False)

    # the CPU LAPACK factorisation in the element type (for fp64: the reference itself)
    def lapack(self):
        if self._lapack is None:
            L = torch.linalg.cholesky(self.K_pad().to(self.dtype))
            W = torch.linalg.solve_triangular(L, torch.eye(self.n_pad, dtype=self.dtype).expand(self.q, -1, -1), upper=False)
            self._lapack = dict(U=L.transpose(1, 2).contiguous(), W=torch.tril(W), L=L)
        return self._lapack

    def z_lapack(self, rhs):
        return torch.linalg.solve_triangular(self.lapack()["L"], self.rhs_pad(rhs).to(self.dtype), upper=False)


def nonpd_matrix(case, latent, k):
    """The matrices of `case` with pivot k of `latent` made -0.5 U_kk^2: K = U_ref^T U_ref with K[k][k] lowered by 1.5 U_ref[k][k]^2
    (rounded to the element type).  Unmistakable in fp32: the first k pivots are those of K, pivot k is negative."""
    U = case.ref()["U"][latent, :case.n, :case.n]
    Kb = U.transpose(0, 1) @ U
    Kb[k, k] -= 1.5 * U[k, k] ** 2
    K = case.K.clone()
    K[latent] = _round(Kb, case.dtype)
    return K


# ------------------------------------------------------------------------------------------------ buffer layout
def _blocks(n_pad):
    return torch.arange(n_pad) // NB


def fill_buffer(ws, K, rhs):
    """Lay K (q, n, n) and rhs (q, naug, n) or None into ws.A the way plmc_assemble / plmc_write_rhs do -- upper 128-tiles, full
    diagonal blocks, the identity on the padded rows n .. n_pad, right-hand sides in the augmented columns with padded rows and
    padded columns zero -- and NaN everywhere else: the strictly lower block tiles of the square part, the whole W region and
    whatever lies behind it."""
    q, n, n_pad = ws.q, ws.n, ws.n_pad
    A = torch.full((q, n_pad, ws.lda), float("nan"), dtype=torch.float64)
    Kp = torch.eye(n_pad, dtype=torch.float64).repeat(q, 1, 1)
    Kp[:, :n, :n] = K
    blk = _blocks(n_pad)
    A[:, :, :n_pad] = torch.where(blk[None, :] >= blk[:, None], Kp, torch.full_like(Kp, float("nan")))
    if ws.naug_pad > 0:
        A[:, :, n_pad:n_pad + ws.naug_pad] = 0.0
        if rhs is not None:
            assert rhs.shape == (q, ws.naug, n)
            A[:, :n, n_pad:n_pad + ws.naug] = rhs.transpose(1, 2)
    ws.A.copy_(A.to(ws.dtype))


def read_factor(ws):
    """-> dict of fp64 host tensors: U = the element-wise upper triangle of A[:, :n_pad, :n_pad], W = the element-wise lower
    triangle of the W columns (None without them), Z = the live augmented columns (q, n_pad, naug), and the raw buffer."""
    A = ws.A.detach().cpu().double()
    n_pad = ws.n_pad
    i = torch.arange(n_pad)
    zero = torch.zeros(())
    out = dict(A=A, U=torch.where(i[None, :] >= i[:, None], A[:, :, :n_pad], zero), W=None,
               Z=A[:, :, n_pad:n_pad + ws.naug].clone())
    if ws.with_inverse:
        out["W"] = torch.where(i[None, :] <= i[:, None], A[:, :, ws.wcol0:ws.wcol0 + n_pad], zero)
    return out


def write_factor(ws, U, W, Z):
    """The "fake sweep": put a finished factorisation into a buffer that fill_buffer prepared, where the sweep puts it --
    U in the upper triangle of the square part, W in its tiles on and below the block diagonal (explicit zeros above the
    diagonal inside the diagonal blocks), Z in the live augmented columns."""
    n_pad = ws.n_pad
    i, blk = torch.arange(n_pad), _blocks(n_pad)
    sq = ws.A[:, :, :n_pad]
    ws.A[:, :, :n_pad] = torch.where(i[None, :] >= i[:, None], U.to(ws.dtype), sq)
    if ws.with_inverse and W is not None:
        wv = ws.A[:, :, ws.wcol0:ws.wcol0 + n_pad]
        ws.A[:, :, ws.wcol0:ws.wcol0 + n_pad] = torch.where(blk[None, :] <= blk[:, None], torch.tril(W).to(ws.dtype), wv)
    if ws.naug > 0 and Z is not None:
        ws.A[:, :, n_pad:n_pad + ws.naug] = Z.to(ws.dtype)
    d = torch.diagonal(ws.A[:, :, :n_pad], dim1=1, dim2=2).double()
    ws.logdet.copy_(2.0 * torch.log(d).sum(-1))
    bad = ~((d > 0) & (d < 3.0e38))
    first = torch.where(bad.any(-1), bad.double().argmax(-1) + 1, torch.zeros((), dtype=torch.int64))
    ws.info.copy_(first.to(torch.int32))


# ------------------------------------------------------------------------------------------------ measures
def _fro(M):
    return torch.linalg.matrix_norm(M)


def _tile_err(M, Mref, denom):
    """max over 128 x 128 tiles of |M - Mref|_F(tile) / denom, and that tile: (q,), list of (ib, jb)"""
    D = M - Mref
    q, r, c = D.shape
    cp = pad(c)
    if cp != c:
        D = torch.cat([D, torch.zeros(q, r, cp - c, dtype=D.dtype, device=D.device)], dim=2)
    t = D.reshape(q, r // NB, NB, cp // NB, NB).pow(2).sum(dim=(2, 4)).sqrt() / denom.reshape(-1, 1, 1)
    flat = t.reshape(q, -1)
    t = torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat)
    e, idx = t.max(dim=1)
    return e, [(int(i) // (cp // NB), int(i) % (cp // NB)) for i in idx.tolist()]


def measures(case, dtype, K_pad, B_pad, fac, ref, z_ref, device="cpu"):
    """All measures of one factorisation `fac` = dict(U, W or None, Z or None) against K_pad (q, n_pad, n_pad), B_pad
    (q, n_pad, naug) or None and the fp64 reference.  Per latent: {name: (q,) tensor}, and {name: tile} for the e measures.
    The products are fp64 on `device` (torch.matmul there is not code under test)."""
    u, n_pad = UNIT[dtype], case.n_pad
    f = lambda t: None if t is None else t.to(device=device, dtype=torch.float64)
    K, B, U, W, Z, Ur, Wr, Zr = (f(t) for t in (K_pad, B_pad, fac["U"], fac.get("W"), fac.get("Z"), ref["U"], ref["W"], z_ref))
    out, tiles = {}, {}
    n = case.n
    lead = lambda M: _fro(M[:, :n, :n])
    nU = lead(U)
    out["rho_U"] = _fro(U.transpose(1, 2) @ U - K) / (n_pad * u * lead(K))
    out["e_U"], tiles["e_U"] = _tile_err(U, Ur, lead(Ur))
    if W is not None:
        eye = torch.eye(n_pad, dtype=torch.float64, device=U.device)
        out["rho_W"] = _fro(W @ U.transpose(1, 2) - eye) / (n_pad * u * nU * lead(W))
        out["e_W"], tiles["e_W"] = _tile_err(W, Wr, lead(Wr))
    if Z is not None and Z.shape[-1] > 0:
        R = U.transpose(1, 2) @ Z - B
        cols = torch.linalg.vector_norm(R, dim=1) / (n_pad * u * nU[:, None] * torch.linalg.vector_norm(Z, dim=1))
        out["rho_Z"] = torch.where(torch.isnan(cols), torch.full_like(cols, float("inf")), cols).max(dim=1).values
        out["e_Z"], tiles["e_Z"] = _tile_err(Z, Zr, _fro(Zr))
    out = {k: torch.where(torch.isnan(v), torch.full_like(v, float("inf")), v).cpu() for k, v in out.items()}
    return out, tiles


def reference_measures(case, rhs, device="cpu"):
    """the measures of the CPU LAPACK factorisation in the element type: rho_ref, e_ref"""
    lap = case.lapack()
    fac = dict(U=lap["U"].double(), W=lap["W"].double(), Z=None if rhs is None else case.z_lapack(rhs).double())
    return measures(case, case.dtype, case.K_pad(), None if rhs is None else case.rhs_pad(rhs), fac, case.ref(),
                    None if rhs is None else case.z_ref(rhs), device)[0]


def e_floor(kappa, n_pad):
    """accuracy of the fp64 reference in the units of the e measures (module docstring)"""
    return kappa ** 1.5 * n_pad * 2.0 ** -53


def plain_thresholds(case, meas_ref, names):
    """{name: (q,) tensor}: (1 + sqrt kappa) max(reference measure, floor)"""
    kap = case.kappa
    margin = 1.0 + torch.sqrt(kap)
    thr = {}
    for k in names:
        floor = torch.ones_like(kap) if k.startswith("rho") else e_floor(kap, case.n_pad)
        thr[k] = margin * torch.maximum(meas_ref[k], floor)
    return thr


def relative(name, v, n_pad, dtype):
    """a measure as a relative quantity: e as it is, rho times n_pad u"""
    return v * (n_pad * UNIT[dtype]) if name.startswith("rho") else v


def split_apriori_rho_u(case, groups):
    """A-priori bound of rho_U for a sweep whose depth-(128 G) products run on a split scheme, in rho units of
    fp32.  Componentwise |U^T U - K| <= c |U|^T |U| with c the sum of
      - the fp32 parts (diagonal blocks, rank-128 updates, the final subtraction and scaling): (n_pad + 1) 2^-24, the classical
        constant of a Cholesky factorisation in that precision,
      - per group product, the two-plane fp16 constants of 3.4: 2 * 2^-23 (operands rounded to 22 bits) + 2^-22 (the dropped
        h1 h1 product) + 2 * 2^-24,
      - one rounding of the level-0 sum per 32 contraction rows over the whole depth: (n_pad / 32) 2^-24
    (the three-plane bf16 scheme splits exactly and drops products of 2^-24 and below: it is inside the same constants).
    Frobenius norms: |U^T U - K|_F <= c | |U_ref|^T |U_ref| |_F."""
    n_pad, u = case.n_pad, UNIT[torch.float32]
    c = (n_pad + 1) * u + groups * (2 * 2.0 ** -23 + 2.0 ** -22 + 2 * u) + (n_pad / 32.0) * u
    Ua = case.ref()["U"].abs()
    return c * _fro(Ua.transpose(1, 2) @ Ua) / (n_pad * u * _fro(case.K))


def violations(meas, thr):
    """[(name, latent, value, threshold)] of every measure above its threshold (inf counts)"""
    bad = []
    for k, t in thr.items():
        v = meas[k]
        for lat in range(v.shape[0]):
            if not float(v[lat]) <= float(t[lat]):
                bad.append((k, lat, float(v[lat]), float(t[lat])))
    return bad


def split_violations(meas_split, meas_plain, n_pad, dtype, names):
    bad = []
    for k in names:
        s, p = relative(k, meas_split[k], n_pad, dtype), relative(k, meas_plain[k], n_pad, dtype)
        for lat in range(s.shape[0]):
            if not float(s[lat]) < 2.0 * float(p[lat]) + 2e-6:
                bad.append((k, lat, float(s[lat]), 2.0 * float(p[lat]) + 2e-6))
    return bad


# ------------------------------------------------------------------------------------------------ the assertions of a sweep
def structure_violations(ws, fac, info, want_info=None):
    """The exact properties of a finished buffer: info, finiteness of everything read, identity / zeros on the padded rows, the
    W contract (finite on and below the block diagonal, the NaN canary of fill_buffer above it).  -> list of strings"""
    bad = []
    n, n_pad, q = ws.n, ws.n_pad, ws.q
    want_info = [0] * q if want_info is None else want_info
    if info.tolist() != list(want_info):
        bad.append("info %s, expected %s" % (info.tolist(), list(want_info)))
    ok = [l for l in range(q) if want_info[l] == 0]
    for name in ("U", "W", "Z"):
        if fac.get(name) is not None and not bool(torch.isfinite(fac[name][ok]).all()):
            bad.append("%s is not finite" % name)
    if n_pad > n:
        i = torch.arange(n_pad)
        rows = fac["U"][ok][:, n:, :]
        if not torch.equal(rows, (i[None, :] == i[n:, None]).double().expand_as(rows)):
            bad.append("padded rows of U are not the identity")
        if fac.get("Z") is not None and fac["Z"].shape[-1] > 0 and not bool((fac["Z"][ok][:, n:, :] == 0).all()):
            bad.append("padded rows of Z are not zero")
    if ws.with_inverse:
        blk = _blocks(n_pad)
        Wraw = fac["A"][ok][:, :, ws.wcol0:ws.wcol0 + n_pad]
        low = (blk[None, :] <= blk[:, None]).expand_as(Wraw)
        if not bool(torch.isfinite(Wraw[low]).all()):
            bad.append("a W tile on or below the block diagonal is not finite")
        if not bool(torch.isnan(Wraw[~low]).all()):
            bad.append("a W tile above the block diagonal was written")
        i = torch.arange(n_pad)
        inside = ((blk[None, :] == blk[:, None]) & (i[None, :] > i[:, None])).expand_as(Wraw)
        if not bool((Wraw[inside] == 0).all()):
            bad.append("W is not zero above the diagonal inside a diagonal block")
    return bad


def logdet_violations(case, dtype, fac, logdet, ok=None):
    """logdet against 2 sum log U_ii of the factor's own diagonal in fp64 -- |d| <= n_pad 2u (one rounding of each pivot) plus
    the floor of ANY fp64 evaluation of that sum of n_pad terms, (n_pad - 1) 2^-53 sum |2 log U_ii| (Higham, Accuracy and
    Stability, 4.2: independent of the order; no double-valued output can do without it: half a unit in the last place of a
    log det of 8000 is already 4.5e-13 > 1152 * 2 * 2^-53; measured on the MI355X, fp64, scale 1e-3, n_pad = 1152: 1.8e-12 = one unit
    in the last place of log det = -9009 against the bare 2.6e-13) -- and against the fp64 reference: |d| <= n_pad u kappa_2(K)."""
    u, n_pad = UNIT[dtype], case.n_pad
    ok = range(case.q) if ok is None else ok
    bad = []
    for l in ok:
        terms = [2.0 * math.log(float(x)) for x in torch.diagonal(fac["U"][l]).tolist()]
        own = math.fsum(terms)
        bound = n_pad * 2 * u + (n_pad - 1) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
        d = abs(float(logdet[l]) - own)
        if d > n_pad * 2 * u:
            print("logdet[%d] = %.6e: |difference to its own diagonal| %.3e is above n_pad 2u = %.3e (summation floor %.3e)"
                  % (l, float(logdet[l]), d, n_pad * 2 * u, bound - n_pad * 2 * u))
        if not d <= bound:
            bad.append("logdet[%d] - 2 sum log U_ii = %.3e > %.3e" % (l, d, bound))
        d = abs(float(logdet[l]) - float(case.ref()["logdet"][l]))
        bound = n_pad * u * float(case.kappa[l])
        if not d <= bound:
            bad.append("logdet[%d] - reference = %.3e > %.3e" % (l, d, bound))
    return bad


def check_sweep(case, ws, rhs, K=None, want_info=None, device="cpu", plain=None, groups=None, logdet=True, rows=None, label=""):
    """Every assertion on one finished buffer `ws` (a sweep's, or a fake one): structure, measures against their thresholds,
    log det.  rhs: the (q, naug, n) right-hand sides that were laid in, or None.  K: the matrices that were laid in where they are
    not case.K.  want_info: expected info per latent (latents that are expected to fail are left out of every other check).
    plain: the measures of the same call under PLMC_SPLIT=0 -- the buffer then comes from a split scheme and is held to the
    split rule and, with `groups` (groups of block rows of that sweep), to the a-priori bound.
    -> (violations: list of strings or (name, latent, value, threshold), measures, tiles).  rows: list that receives one
    (label, measure, latent, value, reference, ratio, tile) per measure for the record in profiles/."""
    q = case.q
    want = [0] * q if want_info is None else list(want_info)
    ok = [l for l in range(q) if want[l] == 0]
    fac = read_factor(ws)
    bad = structure_violations(ws, fac, ws.info.cpu(), want)
    B_pad = case.rhs_pad(rhs) if (rhs is not None and ws.naug > 0) else None
    fac_m = dict(U=fac["U"], W=fac["W"], Z=fac["Z"] if B_pad is not None else None)
    ref = case.ref()
    meas, tiles = measures(case, ws.dtype, case.K_pad(K), B_pad, fac_m, ref, case.z_ref(rhs) if B_pad is not None else None, device)
    key = None if B_pad is None else (tuple(rhs.shape), float(rhs.abs().sum()))
    cache = case.__dict__.setdefault("_ref_meas", {})
    if key not in cache:
        cache[key] = reference_measures(case, rhs if B_pad is not None else None, device)
    ref_meas = cache[key]
    names = list(meas)
    if plain is None:
        mv = violations(meas, plain_thresholds(case, ref_meas, names))
    else:
        mv = split_violations(meas, plain, case.n_pad, ws.dtype, names)
        if groups is not None:
            mv += violations({"rho_U": meas["rho_U"]}, {"rho_U": split_apriori_rho_u(case, groups)})
    bad += [v for v in mv if v[1] in ok]
    if logdet:
        bad += logdet_violations(case, ws.dtype, fac, ws.logdet.cpu(), ok)
    if rows is not None:
        for k in names:
            for l in ok:
                r = float(ref_meas[k][l])
                rows.append((label, k, l, float(meas[k][l]), r, float(meas[k][l]) / r if r > 0 else float("nan"),
                             tiles[k][l] if k in tiles else None))
    return bad, meas, tiles
