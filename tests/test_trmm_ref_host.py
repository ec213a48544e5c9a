"""The reference and the bound of the draw product (tests/_trmm_ref.py) on their own, and the host logic of the draws, without a GPU.

  * a torch-CPU product in the element type, formed from the NaN-laden buffer through the element-wise mask, stays inside the bound at
    every shape tests/test_gpu_trmm_ut.py runs;
  * four seeded mistakes a kernel could make leave it: the strictly lower part of a diagonal block taken along, k < i for k <= i,
    U z for U^T z, the shift dropped;
  * distributions: the shape of get_base_samples for every covariance type, and the two covariances that are not served.
"""
import warnings

import pytest
import torch

import _trmm_ref as tr

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", tr.SIZES)
def test_cpu_product_in_the_element_type_is_inside_the_bound(dtype, n):
    for q in tr.QS:
        for ns in tr.NS:
            for with_shift in (False, True):
                U, Z, shift = tr.make_inputs(n, q, ns, dtype, with_shift=with_shift)
                ws = tr.nan_factor_buffer(n, q, dtype, U)
                Y = tr.cpu_product(ws, n, Z, shift, dtype)
                assert not bool(torch.isnan(Y).any())
                bad = tr.violations(Y, tr.reference(U, Z, shift), tr.bound(U, Z, shift, dtype))
                assert not bad, (n, q, ns, with_shift, bad)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mutate", ["block_lower", "strict", "untransposed", "no_shift"])
def test_seeded_mutations_leave_the_bound(dtype, mutate):
    n, q, ns = 300, 3, 5
    U, Z, shift = tr.make_inputs(n, q, ns, dtype)
    g = torch.Generator().manual_seed(5)
    lower = torch.randn(q, n, n, generator=g, dtype=torch.float64) * torch.tensor(tr.SCALES, dtype=torch.float64).reshape(-1, 1, 1)
    ws = tr.nan_factor_buffer(n, q, dtype, U, lower=lower)          # finite below the diagonal: a wrong mask shows as an error, not as NaN
    Yref, bnd = tr.reference(U, Z, shift), tr.bound(U, Z, shift, dtype)
    assert not tr.violations(tr.cpu_product(ws, n, Z, shift, dtype), Yref, bnd)
    bad = tr.violations(tr.cpu_product(ws, n, Z, shift, dtype, mutate=mutate), Yref, bnd, limit=10 ** 9)
    assert len(bad) > n, (mutate, len(bad))                          # not a stray element: every latent, most rows


def test_nan_below_the_diagonal_reaches_a_product_that_multiplies_by_zero():
    """why the mask has to be a select: 0 * NaN is NaN"""
    n, q, ns = 129, 1, 5
    U, Z, shift = tr.make_inputs(n, q, ns, F32)
    ws = tr.nan_factor_buffer(n, q, F32, U)
    A = ws.A[:, :n, :n]
    Y = (A * torch.triu(torch.ones(n, n))).transpose(1, 2) @ Z.to(F32)
    assert bool(torch.isnan(Y).any())


# ------------------------------------------------------------------------------------------------ host logic of the draws
def _kernel_prior(q=2, n=7, dtype=F32):
    import projectedlmc as plmc
    X = torch.linspace(-1, 1, n, dtype=dtype)[:, None]
    k = plmc.MaternKernel(batch_shape=torch.Size([q]))
    return plmc.MultivariateNormal(torch.zeros(q, n, dtype=dtype), k(X))


def test_base_sample_shapes_for_every_covariance_type():
    import projectedlmc as plmc
    from projectedlmc.distributions import KroneckerSumCovariance
    from projectedlmc.projected import _DiagonalTaskCovariance
    q, n, p = 2, 7, 3
    prior = _kernel_prior(q, n)
    assert prior.get_base_samples().shape == (q, n)
    assert prior.get_base_samples(torch.Size([3, 2])).shape == (3, 2, q, n)
    assert prior.get_base_samples().dtype == torch.float32
    dense = plmc.MultivariateNormal(torch.zeros(q, n, dtype=F64), torch.eye(n, dtype=F64).expand(q, n, n))
    z = dense.get_base_samples(torch.Size([5]))
    assert z.shape == (5, q, n) and z.dtype == F64
    single = plmc.MultivariateNormal(torch.zeros(n), torch.eye(n))
    assert single.get_base_samples(torch.Size([4])).shape == (4, n)
    indep = plmc.MultitaskMultivariateNormal.from_batch_mvn(prior)
    assert indep.get_base_samples(torch.Size([4])).shape == (4, n, q)
    Ht = torch.randn(q, p)
    full = plmc.MultitaskMultivariateNormal(torch.zeros(n, p), KroneckerSumCovariance(Ht, cov=torch.eye(n).expand(q, n, n), eps=0.1))
    assert full.get_base_samples(torch.Size([4])).shape == (4, n, q + p)
    marg = plmc.MultitaskMultivariateNormal(torch.zeros(n, p), KroneckerSumCovariance(Ht, var=torch.ones(q, n), eps=0.1))
    assert marg.get_base_samples().shape == (n, q + p)
    diag = plmc.MultitaskMultivariateNormal(torch.zeros(n, p), _DiagonalTaskCovariance(torch.ones(n, p)))
    assert diag.get_base_samples(torch.Size([2])).shape == (2, n, p)
    flat = plmc.MultitaskMultivariateNormal(torch.zeros(n, p), torch.eye(n * p))
    assert flat.get_base_samples(torch.Size([2])).shape == (2, n, p)
    # seeds and the generator keyword
    torch.manual_seed(3)
    a = prior.get_base_samples(torch.Size([2]))
    torch.manual_seed(3)
    b = prior.get_base_samples(torch.Size([2]))
    assert torch.equal(a, b)
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    assert torch.equal(prior.get_base_samples(generator=g1), prior.get_base_samples(generator=g2))
    assert not torch.equal(a[0], prior.get_base_samples())


def test_base_samples_of_the_wrong_shape_are_refused_before_anything_runs():
    prior = _kernel_prior()
    with pytest.raises(ValueError, match="base_samples"):
        prior.rsample(base_samples=torch.zeros(3, 2, 8))


def test_the_dense_lmc_prior_is_not_served():
    import projectedlmc as plmc
    from projectedlmc.kernels import LazyLmcKernel
    n, p, q = 6, 2, 2
    c = LazyLmcKernel("rbf", torch.zeros(n, 1), torch.ones(q, 1), None, torch.eye(p).expand(q, p, p))
    dist = plmc.MultitaskMultivariateNormal(torch.zeros(n, p), c)
    assert dist.get_base_samples().shape == (n, p)
    with pytest.raises(NotImplementedError, match="LazyLmcKernel"):
        dist.rsample()
    with pytest.raises(NotImplementedError, match="LazyLmcKernel"):
        dist.sample(torch.Size([2]))


def test_the_sgpr_train_mode_prior_is_not_served():
    import projectedlmc as plmc
    n = 12
    X = torch.linspace(-1, 1, n)[:, None]
    y = torch.zeros(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = plmc.ExactGPModel(X, y, plmc.GaussianLikelihood(), mean_type=plmc.ZeroMean, kernel_type=plmc.RBFKernel, n_inducing_points=4)
    dist = model.forward(X)
    c = dist.lazy_covariance_matrix
    assert hasattr(c, "log_prob_batch")
    with pytest.raises(NotImplementedError, match=type(c).__name__):
        dist.rsample()
    with pytest.raises(NotImplementedError, match=type(c).__name__):
        model.likelihood(dist).sample()
