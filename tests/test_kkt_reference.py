"""CPU check of the KKT-solve reference (tests/_kkt_reference.py) that the direct-solve GPU tests measure against: on a
small K whose exact solution is computed in rational arithmetic, the refined solution must be far closer to it than
numpy's plain float64 solve, at cond(K) = 1e0, 1e6 and 1e10."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import sparse

from tests._kkt_reference import KKTReference, reduced_matrix, rel_err


def _exact_solution(P_upper, A, sigma, rho, b):
    """x = K^-1 (b1 + A'(rho . b2)) in exact rational arithmetic from the float64 data (Gauss-Jordan on Fractions)."""
    Pu = sparse.csc_matrix(P_upper).toarray()
    Ad = sparse.csc_matrix(A).toarray()
    n, m = Pu.shape[0], Ad.shape[0]
    F = lambda v: Fraction(float(v))
    P = [[F(Pu[min(i, j), max(i, j)]) for j in range(n)] for i in range(n)]
    Af = [[F(Ad[i, j]) for j in range(n)] for i in range(m)]
    rf = [F(r) for r in rho]
    sg = F(sigma)
    K = [[P[i][j] + (sg if i == j else 0) + sum(Af[k][i] * rf[k] * Af[k][j] for k in range(m)) for j in range(n)] for i in range(n)]
    rhs = [F(b[i]) + sum(Af[k][i] * rf[k] * F(b[n + k]) for k in range(m)) for i in range(n)]
    for p in range(n):
        piv = K[p][p]
        inv = 1 / piv
        K[p] = [v * inv for v in K[p]]
        rhs[p] *= inv
        for i in range(n):
            if i != p and K[i][p] != 0:
                f = K[i][p]
                K[i] = [a - f * c for a, c in zip(K[i], K[p])]
                rhs[i] -= f * rhs[p]
    x = rhs
    z = [sum(Af[k][j] * x[j] for j in range(n)) for k in range(m)]
    return x, z


def _ld(v):
    """A Fraction rounded to long double (two float64 parts: the head and the rounded remainder)."""
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - Fraction(hi)))


def _system(n, m, cond, seed):
    """P = Q diag(logspace) Q' with cond(P) = cond, A with m short rows at small weight: cond(K) ~ cond."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(cond), n) if cond > 1 else np.ones(n)
    P = (Q * lam) @ Q.T
    P = 0.5 * (P + P.T)
    A = sparse.random(m, n, density=0.2, random_state=seed, data_rvs=rng.standard_normal, format="csc")
    rho = np.full(m, 1e-6 / cond)
    return sparse.triu(sparse.csc_matrix(P), format="csc"), A, 1e-3 / cond if cond > 1 else 0.0, rho, rng


@pytest.mark.parametrize("cond", [1e0, 1e6, 1e10])
def test_refined_reference_beats_plain_numpy(cond):
    n, m = 24, 8
    Pu, A, sigma, rho, rng = _system(n, m, cond, seed=int(np.log10(cond)) + 3)
    K = reduced_matrix(Pu, A, sigma, rho)
    c = np.linalg.cond(K)
    assert cond / 10 <= c <= cond * 10, c
    ref = KKTReference(Pu, A, sigma, rho)
    for _ in range(2):
        b = rng.standard_normal(n + m)
        x, z, plain = ref.solve(b)
        xe, ze = _exact_solution(Pu, A, sigma, rho, b)
        exact = np.array([_ld(v) for v in xe + ze], dtype=np.longdouble)
        # the exact rational solution rounded to long double is the yardstick: the refined solution to near long-double
        # accuracy (cond x 2^-64), numpy's plain solve to cond x 2^-53 at best
        refined_err = rel_err(ref.last, exact)
        plain_err = rel_err(np.concatenate([np.linalg.solve(K, ref.rhs(b).astype(float)), A @ np.linalg.solve(K, ref.rhs(b).astype(float))]), exact)
        print(f"cond {c:.1e}: refined {refined_err:.2e}, plain numpy {plain_err:.2e} (helper's own estimate {plain:.2e})")
        assert refined_err <= max(1e-2 * plain_err, 1e-17), (refined_err, plain_err)
        # the helper's estimate of numpy's error is that error, measured against a solution this much better
        assert abs(plain - plain_err) <= 1e-2 * plain_err + 1e-17, (plain, plain_err)
        # and the float64 copies it returns are the refined values rounded
        assert rel_err(np.concatenate([x, z]), exact) <= refined_err + 2.0 ** -52
        assert ref.forward_error(np.concatenate([x, z])) <= 2.0 ** -52


def test_residual_of_refined_solution_is_at_roundoff():
    Pu, A, sigma, rho, rng = _system(40, 15, 1e8, seed=7)
    ref = KKTReference(Pu, A, sigma, rho)
    b = rng.standard_normal(55)
    ref.solve(b)
    refined = ref.residual(ref.last[:40], b)
    plain = ref.residual(np.linalg.solve(ref.K, ref.rhs(b).astype(float)), b)
    assert refined <= 1e-2 * plain, (refined, plain)
