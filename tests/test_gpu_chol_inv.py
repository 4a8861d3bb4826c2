"""GPU: ``capi.chol_inv_transposed`` -- the one-workgroup Cholesky factor and triangular inverse of the spectral order's subspace iteration
(voltrix/reorder_kernels.hpp) -- against the same operation in numpy float64:

    S = 0.5 (G + G^T) + eps trace(G) I   (double, from the fp32 G),   L = cholesky(S),   ref = inv(L)^T

k = 1 (one thread), 2, 7, 31 / 32 / 33 (the comment's k = 32 and both sides of it), 63, 64 (the last row of the 64-thread workgroup);
eps = 1e-10 and 0; G = X^T X of a seeded Gaussian X [4 k, k] (the float64 product rounded once to fp32, so that every machine tests the
same G), and the same G plus a small skew part, which only a kernel that symmetrises handles like the reference.

Bound, per element:  |out - ref| <= 2^-24 |ref| + k 2^-50 kappa max|ref|.  The first term is the one rounding of the kernel's double result
to fp32; the second covers double arithmetic in another order than LAPACK's (kappa = the float64 condition number of S, computed here and
asserted < 1e4 for these inputs -- it is 1 .. 9.3 -- so that the second term stays far below the first).  Derived, not measured.

Every call runs on output memory filled with 0xFF bytes (NaN); k = 0 and k = 65 are refusals: tests/core_abi_cases.py."""
import numpy as np
import pytest

from poisoned_alloc import poisoned

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 31, 32, 33, 63, 64)
EPS = (1e-10, 0.0)


def _x(k, seed=0):
    return np.random.default_rng(1000 * seed + k).standard_normal((4 * k, k)).astype(np.float32)


def _gram(x):
    x64 = x.astype(np.float64)
    return (x64.T @ x64).astype(np.float32)


def _skewed(g, k):
    a = np.random.default_rng(77 + k).standard_normal((k, k))
    return (g.astype(np.float64) + 1e-3 * (a - a.T)).astype(np.float32)


def _shifted(g32, eps):
    g = g32.astype(np.float64)
    return 0.5 * (g + g.T) + eps * np.trace(g) * np.eye(g.shape[0]), eps * np.trace(g)


def _inv_transposed(lower):
    from scipy.linalg import solve_triangular

    return solve_triangular(lower, np.eye(lower.shape[0]), lower=True).T


def _reference(g32, eps):
    """``(ref, kappa)`` in float64."""
    s, _ = _shifted(g32, eps)
    return _inv_transposed(np.linalg.cholesky(s)), float(np.linalg.cond(s))


def _reference_with_replaced_pivots(g32, eps):
    """The header's rule for a rank-deficient subspace as a plain float64 loop: column-by-column Cholesky, a pivot <= 0 replaced by
    eps trace, or by 1e-300 when that is not positive.  ``(ref, S)``."""
    s, shift = _shifted(g32, eps)
    a, k = s.copy(), s.shape[0]
    for j in range(k):
        d = a[j, j] if a[j, j] > 0.0 else (shift if shift > 0.0 else 1e-300)
        a[j, j] = np.sqrt(d)
        for t in range(j + 1, k):
            a[t, j] /= a[j, j]
        for t in range(j + 1, k):
            for c in range(j + 1, t + 1):
                a[t, c] -= a[t, j] * a[c, j]
    return _inv_transposed(np.tril(a)), s


def _bound(ref, k, kappa, scale=None):
    return 2.0 ** -24 * np.abs(ref) + k * 2.0 ** -50 * kappa * (np.abs(ref).max() if scale is None else scale)


def _run(g32, eps, stream=None):
    """The kernel on ``g32`` with its output allocated from memory of 0xFF bytes; float64 numpy."""
    import torch

    from voltrix import capi

    gram = torch.from_numpy(g32).cuda()
    torch.cuda.synchronize()
    with poisoned(0xFF) as state:
        if stream is None:
            out = capi.chol_inv_transposed(gram, eps)
        else:
            with torch.cuda.stream(stream):
                out = capi.chol_inv_transposed(gram, eps, stream=stream.cuda_stream)
            stream.synchronize()
    assert state.filled == 1 and out.dtype == torch.float32 and tuple(out.shape) == g32.shape
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def _check(out, ref, k, kappa, what):
    assert np.isfinite(out).all(), what
    assert (np.tril(out, -1) == 0.0).all(), f"{what}: an element below the diagonal is not exactly 0"
    ratio = float((np.abs(out - ref) / _bound(ref, k, kappa)).max())
    print(f"chol_inv_transposed {what}: kappa {kappa:.3g}, worst |out - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst |out - ref| / bound = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("k", SIZES)
def test_against_float64_cholesky(cuda_device, k, eps):
    x = _x(k)
    g = _gram(x)
    ref, kappa = _reference(g, eps)
    assert kappa < 1e4, kappa
    out = _run(g, eps)
    _check(out, ref, k, kappa, f"k={k} eps={eps}")
    q = x.astype(np.float64) @ out                            # X out has orthonormal columns: two fp32-rounded factors
    gap = float(np.abs(q.T @ q - np.eye(k)).max())
    print(f"chol_inv_transposed k={k} eps={eps}: max |(X out)^T (X out) - I| = {gap:.3g} (allowed {k * 2.0 ** -22:.3g})")
    assert gap <= k * 2.0 ** -22, gap


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("k", SIZES)
def test_a_non_symmetric_gram_is_symmetrised(cuda_device, k, eps):
    """G plus a skew part of 1e-3: 0.5 (G + G^T) is what is factored -- a kernel that read one triangle of G would be off by 1e-3 / k,
    four orders of magnitude above the bound."""
    g = _skewed(_gram(_x(k)), k)
    assert k == 1 or np.abs(g - g.T).max() > 1e-4
    ref, kappa = _reference(g, eps)
    assert kappa < 1e4, kappa
    _check(_run(g, eps), ref, k, kappa, f"skewed k={k} eps={eps}")


@pytest.mark.parametrize("k", (2, 32, 64))
def test_rank_deficient_subspace(cuda_device, k):
    """Column k - 1 of X equal to column 0, eps = 1e-10: the last pivot is what the shift and cancellation leave of it.  ``out`` is finite
    everywhere, and columns 0 .. k - 2 -- rows 0 .. k - 2 of inv(L), which depend on the leading (k - 1) x (k - 1) block of S alone --
    meet the bound with the condition number of THAT block (S itself has kappa of about 1 / eps; the block's is that of the random
    inputs) and the largest reference element among those columns.  The last column divides by the replaced or cancelled pivot: its
    size is not compared."""
    x = _x(k, seed=1)
    x[:, k - 1] = x[:, 0]
    g = _gram(x)
    eps = 1e-10
    ref, s = _reference_with_replaced_pivots(g, eps)
    kappa = float(np.linalg.cond(s[:k - 1, :k - 1]))
    assert kappa < 1e4 and np.linalg.cond(s) > 1e8, (kappa, np.linalg.cond(s))
    out = _run(g, eps)
    assert np.isfinite(out).all() and (np.tril(out, -1) == 0.0).all()
    lead = ref[:, :k - 1]
    ratio = float((np.abs(out[:, :k - 1] - lead) / _bound(lead, k, kappa)).max())
    print(f"chol_inv_transposed rank-deficient k={k}: block kappa {kappa:.3g}, worst |out - ref| / bound = {ratio:.3f}, "
          f"last column max |out| = {np.abs(out[:, k - 1]).max():.3g}")
    assert ratio <= 1.0, ratio


def test_on_a_side_stream(cuda_device):
    import torch

    k, eps = 33, 1e-10
    g = _gram(_x(k))
    ref, kappa = _reference(g, eps)
    _check(_run(g, eps, stream=torch.cuda.Stream()), ref, k, kappa, f"side stream k={k}")
