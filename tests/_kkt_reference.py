"""Reference for one reduced KKT solve (what hipeng_kkt_solve / LinSysSolver.solve return), for the direct-solve tests.

Given triu(P), A, sigma, a rho vector and b = [b1; b2]:
    K = P + sigma I + A' diag(rho) A,   x~ = K^-1 (b1 + A'(rho . b2)),   z~ = A x~.
The system is solved in float64 by LAPACK's LU with partial pivoting on the dense K (what np.linalg.solve does), then improved by a few steps of
iterative refinement whose residuals are formed in np.longdouble with K applied as an operator,
P x + sigma x + A'(rho . (A x)), over long-double copies of P and A (K itself is never formed in long double).

The error that plain float64 numpy makes on the same system (no refinement) comes back too, and inverse_error() gives that of
the float64 inverse of K applied to the right-hand side: the GPU bars are scaled by them.
"""
import numpy as np
import scipy.linalg as sla
from scipy import sparse

LD = np.longdouble


def full_p(P_upper):
    """The symmetric P from its upper triangle."""
    Pu = sparse.csc_matrix(P_upper)
    return (Pu + sparse.triu(Pu, 1, format="csc").T).tocsc()


def reduced_matrix(P_upper, A, sigma, rho):
    """K = P + sigma I + A' diag(rho) A as a dense float64 array."""
    P = full_p(P_upper)
    A = sparse.csc_matrix(A)
    n = P.shape[0]
    K = (P + sigma * sparse.eye(n, format="csc") + A.T @ sparse.diags(np.asarray(rho, float)) @ A).toarray()
    return K


def rel_err(a, ref):
    """Relative infinity-norm error  max|a - ref| / max|ref|."""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    den = np.abs(ref).max()
    return float(np.abs(a - ref).max() / den) if den > 0 else float(np.abs(a).max())


class KKTReference:
    """The refined solve of one (P, A, sigma, rho).  K is formed and factored once; solve() takes any right-hand side."""

    def __init__(self, P_upper, A, sigma, rho, K=None):
        P = full_p(P_upper)
        self.n = P.shape[0]
        self.A = sparse.csr_matrix(A)
        self.m = self.A.shape[0]
        self.sigma = float(sigma)
        self.rho = np.asarray(rho, dtype=float)
        self.K = reduced_matrix(P_upper, A, sigma, rho) if K is None else K
        self.lu = sla.lu_factor(self.K, check_finite=False)
        # long-double operator copies (sparse storage: only the arithmetic is long double)
        self.Pl = sparse.csr_matrix(P).astype(LD)
        self.Al = self.A.astype(LD)
        self.AlT = self.Al.T.tocsr()
        self.rhol = self.rho.astype(LD)
        self.sigmal = LD(self.sigma)

    def apply(self, x):
        """K x in long double."""
        x = np.asarray(x, dtype=LD)
        out = self.Pl @ x + self.sigmal * x
        if self.m:
            out = out + self.AlT @ (self.rhol * (self.Al @ x))
        return out

    def rhs(self, b):
        """b1 + A'(rho . b2) in long double."""
        b = np.asarray(b, dtype=LD)
        r = b[: self.n].copy()
        if self.m:
            r = r + self.AlT @ (self.rhol * b[self.n:])
        return r

    def solve(self, b, steps=3):
        """Returns (x~, z~, plain_err): the refined solution (float64 copies of long-double values) and the relative
        infinity-norm error of numpy's plain float64 [x~; z~] against it."""
        rl = self.rhs(b)
        x_plain = sla.lu_solve(self.lu, rl.astype(float), check_finite=False)      # (np.linalg.solve: the same getrf + getrs)
        x = x_plain.astype(LD)
        for _ in range(steps):
            res = rl - self.apply(x)
            x = x + sla.lu_solve(self.lu, res.astype(float), check_finite=False).astype(LD)
        z = self.Al @ x if self.m else np.zeros(0, dtype=LD)
        ref = np.concatenate([x, z])
        plain = np.concatenate([x_plain, self.A @ x_plain]).astype(LD)
        self.last = ref
        return x.astype(float), z.astype(float), rel_err(plain, ref)

    def inverse_error(self, b):
        """Relative infinity-norm error of [x~; z~] when the float64 inverse of K (LAPACK, from the LU factors) multiplies the
        whole right-hand side: what applying an explicit inverse costs even when that inverse is accurate to roundoff.  Call
        after solve(b)."""
        if not hasattr(self, "Kinv"):
            self.Kinv = sla.lu_solve(self.lu, np.eye(self.n), check_finite=False)
        x = self.Kinv @ self.rhs(b).astype(float)
        return rel_err(np.concatenate([x, self.A @ x]).astype(LD), self.last)

    def forward_error(self, xz):
        """Relative infinity-norm error of a float64 [x~; z~] against the last refined solution."""
        return rel_err(xz, self.last)

    def residual(self, x, b):
        """||rhs - K x|| / ||rhs|| (infinity norms, long double)."""
        rl = self.rhs(b)
        return float(np.abs(rl - self.apply(x)).max() / np.abs(rl).max())
