"""The bordered update of a finished factorisation (csrc/factor_extend.hip) restated in torch on the CPU, and the
buffers its tests share.  Nothing here imports the library or touches a GPU.

Per latent, from the factor U (upper, Khat = U^T U) and inverse factor W = U^-T (lower) of the leading n x n block and m new points:
    V = W K12,  S = K22 - V^T V,  U22 = chol(S)^T,  W22 = U22^-T,  B = W^T V,  W21 = -W22 B^T,
    U' = [[U, V], [0, U22]],  W' = [[W, 0], [W21, W22]].
Every product is formed in the ELEMENT TYPE, as the library forms it; S, its Cholesky factor and its inverse are fp64 and rounded once.
The Cholesky factor is unique, so U', W' are judged by tests/_factor_ref.py with the rules of the sweep, on Case(family, n + m, ...):
the leading n x n block of that case's matrix is the matrix whose factor is extended.

SHAPES: single new row; across a block edge (n_pad 256 -> 384); first row of a new block; inside the old padding; full width; across the
first block edge; two calls (128, then 1 in place)."""
import torch

import _factor_ref as fr

NB = fr.NB
SHAPES = [(300, 1), (250, 10), (256, 1), (200, 40), (130, 128), (127, 2), (383, 129)]
MUTATIONS = ("w21_sign", "s_without_vtv", "old_identity", "b_with_u")


def leading_factor(case, n):
    """(U, W) of the leading n x n block of case.K: the CPU LAPACK factorisation in the element type, (q, n, n) each"""
    L = torch.linalg.cholesky(case.K[:, :n, :n].to(case.dtype))
    W = torch.linalg.solve_triangular(L, torch.eye(n, dtype=case.dtype).expand(case.q, -1, -1), upper=False)
    return L.transpose(1, 2).contiguous(), torch.tril(W)


def _pad_identity(M, n_pad):
    q, n = M.shape[0], M.shape[1]
    out = torch.eye(n_pad, dtype=M.dtype).repeat(q, 1, 1)
    out[:, :n, :n] = M
    return out


def source_workspace(case, n, naug, ws_cls=fr.HostWorkspace, **kw):
    """A workspace of n live rows holding the element-type LAPACK factor of the leading block where a sweep would leave it, NaN wherever
    fill_buffer leaves NaN; the augmented block is zero.  ws_cls(n, q, naug, dtype, ...): HostWorkspace, or the engine's Workspace."""
    ws = ws_cls(n, case.q, naug, case.dtype, **kw)
    host = fr.HostWorkspace(n, case.q, naug, case.dtype, True)
    assert (host.n_pad, host.lda, host.wcol0) == (ws.n_pad, ws.lda, ws.wcol0)
    U, W = leading_factor(case, n)
    fr.fill_buffer(host, case.K[:, :n, :n], None)
    fr.write_factor(host, _pad_identity(U, host.n_pad), _pad_identity(W, host.n_pad), None)
    ws.A.copy_(host.A)
    ws.logdet.copy_(host.logdet)
    ws.info.copy_(host.info)
    return ws


def extend(U, W, K12, K22, mutation=None):
    """One bordered step in the element type of U: (U', W', 2 sum log diag U22).  K12 (q, n, m), K22 (q, m, m) in fp64, rounded here."""
    dt = U.dtype
    q, n, m = K12.shape
    V = W @ K12.to(dt)
    G = V.transpose(1, 2) @ V
    S = K22.to(dt).double() - (0.0 if mutation == "s_without_vtv" else G.double())
    L22 = torch.linalg.cholesky(S)
    W22 = torch.linalg.solve_triangular(L22, torch.eye(m, dtype=torch.float64).expand(q, -1, -1), upper=False)
    B = (U if mutation == "b_with_u" else W).transpose(1, 2) @ V
    W21 = W22.to(dt) @ B.transpose(1, 2)
    if mutation != "w21_sign":
        W21 = -W21
    Ue = torch.zeros(q, n + m, n + m, dtype=dt)
    We = torch.zeros(q, n + m, n + m, dtype=dt)
    Ue[:, :n, :n], Ue[:, :n, n:], Ue[:, n:, n:] = U, V, L22.transpose(1, 2).to(dt)
    We[:, :n, :n], We[:, n:, :n], We[:, n:, n:] = W, W21, torch.tril(W22).to(dt)
    return Ue, We, 2.0 * torch.log(torch.diagonal(L22, dim1=1, dim2=2)).sum(-1)


def extend_in_chunks(case, n, mutation=None):
    """The leading factor of `case` extended to all case.n rows in chunks of at most 128 rows, as the host loops: (U', W')"""
    U, W = leading_factor(case, n)
    k = n
    while k < case.n:
        c = min(NB, case.n - k)
        U, W, _ = extend(U, W, case.K[:, :k, k:k + c], case.K[:, k:k + c, k:k + c], mutation)
        k += c
    return U, W


def extended_workspace(case, n, mutation=None):
    """HostWorkspace of case.n live rows holding the extended factor where plmc_factor_extend leaves it (fake call)"""
    U, W = extend_in_chunks(case, n, None if mutation == "old_identity" else mutation)
    ws = fr.HostWorkspace(case.n, case.q, 1, case.dtype, True)
    fr.fill_buffer(ws, case.K, None)
    fr.write_factor(ws, _pad_identity(U, ws.n_pad), _pad_identity(W, ws.n_pad), None)
    if mutation == "old_identity":
        # the rows of the block that straddles n keep the source's padding identity: what a plain copy of the source would leave
        hi = min(fr.pad(n), case.n)
        assert hi > n, "old_identity needs an n inside a block"
        j = torch.arange(ws.n_pad)
        for i in range(n, hi):
            ws.A[:, i, :ws.n_pad] = torch.where(j >= i, (j == i).to(case.dtype), ws.A[:, i, :ws.n_pad])
        d = torch.diagonal(ws.A[:, :, :ws.n_pad], dim1=1, dim2=2).double()
        ws.logdet.copy_(2.0 * torch.log(d).sum(-1))
    return ws
