"""numpy model of the ADMM loop of config 2 around its linear solve: what a better PCG start vector could save, and how often the
last trip of a resident solve can be called in advance.  Plain numpy / scipy, no GPU, no oracle.

The loop is the engine's: the seeded QP of osqp_amd.problems.random_sparse_qp, 10 Ruiz passes, rho = 0.1, sigma = 1e-6,
alpha = 1.6, the reduced system K = P + sigma I + rho A'A solved by Jacobi-preconditioned CG to ||r|| <= 1e-9 ||b||, the start
vector x~_k + theta (x~_k - x~_{k-1}) with theta = 0 before iteration 5, 1/2 before iteration 12, 1 from there on; rho constant.

  table 1   mean PCG iterations per solve over --iters ADMM iterations for five start vectors: the engine's two-point
            extrapolation, that plus a projection of the start residual on a K-orthonormal basis of the last 8 / 16 PCG
            corrections (x~ - start), a three-point extrapolation, and the plain warm start.
  table 2   the rule of k_pcg_resident on the residual norms of --solves solves with the engine's start vector: after iteration
            i >= 2 predict ||r_i||^2 as ||r_{i-1}||^4 / ||r_{i-2}||^2 and call the next trip the last if that is <= margin tol^2
            (first firing only: one prediction per solve).  Correct: the called trip is the one that learns "converged".

  usage: python tools/pcg_start_model.py [--n 10000] [--m 20000] [--iters 100] [--solves 125]"""
import argparse
import os
import sys

import numpy as np
from scipy import sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from osqp_amd.problems import random_sparse_qp      # noqa: E402  (a data generator: numpy / scipy only)

RHO, SIGMA, ALPHA, STOP = 0.1, 1e-6, 1.6, 1e-9
EX_H0, EX_H1 = 5, 12


def ruiz(P, q, A, l, u, passes=10):
    """OSQP's modified Ruiz equilibration of [[P, A'], [A, 0]] with its cost scaling; returns the scaled problem."""
    n, m = P.shape[0], A.shape[0]
    P, A, q = P.tocsc().copy(), A.tocsc().copy(), q.copy()
    D, E, c = np.ones(n), np.ones(m), 1.0
    lim = lambda v: np.clip(np.where(v < 1e-4, 1.0, v), 1e-4, 1e4)
    for _ in range(passes):
        cn = np.maximum(abs(P).max(axis=0).toarray().ravel(), abs(A).max(axis=0).toarray().ravel())
        rn = abs(A).max(axis=1).toarray().ravel()
        d, e = 1.0 / np.sqrt(lim(cn)), 1.0 / np.sqrt(lim(rn))
        Dm, Em = sparse.diags(d), sparse.diags(e)
        P, A, q = (Dm @ P @ Dm).tocsc(), (Em @ A @ Dm).tocsc(), d * q
        D, E = D * d, E * e
        pn = float(np.mean(abs(P).max(axis=0).toarray().ravel()))
        g = 1.0 / float(lim(np.array([max(pn, np.abs(q).max())]))[0])
        P, q, c = P * g, q * g, c * g
    return P, q, A, l * E, u * E


def pcg(K, minv, b, x, tol2_rel=STOP * STOP, cap=500):
    """Jacobi PCG from x; returns x, iterations, and ||r_i||^2 for i = 0 .. iterations."""
    r = b - K @ x
    tol2 = tol2_rel * float(b @ b)
    rr = [float(r @ r)]
    z = minv * r
    p, rz, it = z.copy(), float(r @ z), 0
    while rr[-1] > tol2 and it < cap:
        Kp = K @ p
        a = rz / float(p @ Kp)
        x = x + a * p
        r = r - a * Kp
        rr.append(float(r @ r))
        z = minv * r
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it, rr, tol2


class Basis:
    """K-orthonormal basis of the last `size` PCG corrections (modified Gram-Schmidt in the K inner product)."""

    def __init__(self, K, size):
        self.K, self.size, self.raw = K, size, []
        self.V = None

    def add(self, d):
        self.raw = (self.raw + [d])[-self.size:]
        V = []
        for v in reversed(self.raw):                 # latest first
            v = v.copy()
            for w in V:
                v -= float(w @ (self.K @ v)) * w
            nk = float(v @ (self.K @ v))
            if nk > 1e-30 * max(1.0, float(v @ v)):
                V.append(v / np.sqrt(nk))
        self.V = np.array(V) if V else None

    def project(self, b, x):
        if self.V is None:
            return x
        return x + self.V.T @ (self.V @ (b - self.K @ x))


def run(P, q, A, l, u, iters, start="two", basis=0):
    """`iters` ADMM iterations; returns per solve the iteration count and the ||r||^2 sequence with its tol^2."""
    n, m = P.shape[0], A.shape[0]
    Pf = (P + sparse.triu(P, 1).T).tocsr()
    K = (Pf + SIGMA * sparse.eye(n) + RHO * (A.T @ A)).tocsr()
    minv = 1.0 / K.diagonal()
    At = A.T.tocsr()
    A = A.tocsr()
    x, z, y = np.zeros(n), np.zeros(m), np.zeros(m)
    hist, out = [], []
    bs = Basis(K, basis) if basis else None
    for k in range(iters):
        b = SIGMA * x - q + At @ (RHO * z - y)
        th = 0.0 if k < EX_H0 else (0.5 if k < EX_H1 else 1.0)
        if not hist:
            s = x.copy()
        elif start == "none" or len(hist) < 2:
            s = hist[-1].copy()
        elif start == "three" and len(hist) >= 3 and th == 1.0:
            s = 3.0 * hist[-1] - 3.0 * hist[-2] + hist[-3]
        else:
            s = hist[-1] + th * (hist[-1] - hist[-2])
        if bs is not None:
            s = bs.project(b, s)
        xt, it, rr, tol2 = pcg(K, minv, b, s)
        if bs is not None and it > 0:
            bs.add(xt - s)
        out.append((it, rr, tol2))
        hist = (hist + [xt])[-3:]
        zt = A @ xt
        xn = ALPHA * xt + (1.0 - ALPHA) * x
        v = ALPHA * zt + (1.0 - ALPHA) * z
        zn = np.clip(v + y / RHO, l, u)
        y = y + RHO * (v - zn)
        x, z = xn, zn
    return out


def predict(rr, tol2, margin):
    """What the rule does on one solve: 'hit', 'early' (called a trip that was not the last), 'none' (did not fire)."""
    N = len(rr) - 1                      # trip t = 1 .. N + 1 sees rr[t - 1]; trip N + 1 learns "converged"
    for t in range(2, N + 1):            # after the update of trip t (which went on)
        if rr[t - 1] * rr[t - 1] <= margin * tol2 * rr[t - 2]:
            return "hit" if t == N else "early"
    return "none"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--solves", type=int, default=125)
    ap.add_argument("--skip-starts", action="store_true", help="table 2 only")
    a = ap.parse_args()
    pb = random_sparse_qp(a.n, a.m, seed=1)
    P, q, A, l, u = ruiz(pb["P"], pb["q"], pb["A"], pb["l"], pb["u"])
    print(f"model: n = {a.n}, m = {a.m}, rho = {RHO}, sigma = {SIGMA}, alpha = {ALPHA}, stop {STOP} ||b||, extrapolation schedule {EX_H0}/{EX_H1}")
    if not a.skip_starts:
        print(f"\nmean PCG iterations per solve, {a.iters} ADMM iterations at constant rho")
        for name, kw in (("two-point extrapolation (the engine)", dict(start="two")),
                         ("plus a K-orthonormal basis of the last 8 corrections", dict(start="two", basis=8)),
                         ("plus a basis of the last 16 corrections", dict(start="two", basis=16)),
                         ("three-point extrapolation", dict(start="three")),
                         ("no extrapolation", dict(start="none"))):
            its = [it for it, _, _ in run(P, q, A, l, u, a.iters, **kw)]
            print(f"  {name:55s} {np.mean(its):6.2f}   (last 50: {np.mean(its[-50:]):.2f})")
    sol = run(P, q, A, l, u, a.solves, start="two")
    print(f"\nthe predicted last trip on {a.solves} solves (mean {np.mean([s[0] for s in sol]):.2f} PCG iterations)")
    print("  threshold     called correctly   one or more trips early   did not fire")
    for margin in (1.0, 0.5, 0.25):
        got = [predict(rr, tol2, margin) for _, rr, tol2 in sol]
        print(f"  {margin:4.2f} tol^2   {got.count('hit'):16d}   {got.count('early'):23d}   {got.count('none'):12d}")
    ratios = [rr[i + 1] / rr[i] for _, rr, _ in sol[20:] for i in range(len(rr) - 1)]
    print(f"  (||r_i||^2 / ||r_(i-1)||^2 over the solves after the 20th: median {np.median(ratios):.3f}, 10 % .. 90 % {np.quantile(ratios, 0.1):.3f} .. {np.quantile(ratios, 0.9):.3f})")


if __name__ == "__main__":
    main()
