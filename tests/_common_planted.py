"""Planted QPs for the common-K engine: one P and one A for the batch, and one class per row for the batch, as the
engine demands -- which _planted_qp._plant does not give (it draws free and one-sided rows per member).

Per case the class of every row is drawn once: equality rows (active in every member, with a multiplier of either
sign), free rows (never active, both bounds infinite in every member) and inequality rows (active or not per member;
one- or two-sided bounds, which are one class).  Per member x*, y* and the active inequality rows are chosen, q and the
bounds follow: |y*| in [0.5, 2] on active rows, every inactive finite bound 0.5 .. 1 away.  Active rows have one row
per variable at most (choose_rows), so they are independent.  The cases are namespaces of the shape _planted_qp.member,
truth and model take (Px_all / Ax_all repeat the shared values)."""
from types import SimpleNamespace

import numpy as np
from scipy import sparse

import _planted_qp as pq

CASES = ("zero", "ns_exact", "vertex", "lp", "no_p", "rows")
NO_P, DENSE_A, EMPTY_COL = (5, 7), (3, 17), 150
_cases = {}


def _plant_member(rng, P, A, eq, free, active_ineq):
    m, n = A.shape
    Pf = (P + sparse.triu(P, 1).T).tocsr()
    x = rng.standard_normal(n)
    act = np.zeros(m, np.int64)
    rows = np.concatenate([eq, active_ineq]).astype(np.int64)
    act[rows] = rng.choice((-1, 1), rows.size)
    y = np.where(act != 0, act * rng.uniform(0.5, 2.0, m), 0.0)
    q = -(Pf @ x + A.T @ y)
    ax = A @ x
    l = ax - rng.uniform(0.5, 1.0, m); u = ax + rng.uniform(0.5, 1.0, m)
    one_sided = rng.random(m) < 0.4                    # of the inequality rows: the bound away from x* is infinite
    for i in range(m):
        if i in free:
            l[i], u[i] = -np.inf, np.inf
        elif act[i] == 0:
            if one_sided[i]:
                if rng.random() < 0.5: l[i] = -np.inf
                else: u[i] = np.inf
        elif act[i] < 0:
            l[i] = ax[i]
            if i in eq: u[i] = ax[i]
            elif one_sided[i]: u[i] = np.inf
        else:
            u[i] = ax[i]
            if i in eq: l[i] = ax[i]
            elif one_sided[i]: l[i] = -np.inf
    return q, l, u, x, y, act


def _assemble(name, seed, n, m, n_eq, counts, n_free=3, must=(), never=(), p_kw=None, a_kw=None):
    """counts: active inequality rows per member.  The candidate rows (one per variable at most) are drawn once; the
    first n_eq of them (`must` first) are the equality rows, every member picks its active inequality rows among the rest."""
    rng = np.random.default_rng(seed)
    P = pq._p_pattern(rng, n, **(p_kw or {}))
    A = pq._a_pattern(rng, n, m, **(a_kw or {}))
    cand = pq.choose_rows(rng, n, m, n_eq + max(counts), must=must, never=never)
    rest = [r for r in cand if r not in must]
    eq = np.array(list(must) + rest[:n_eq - len(must)], np.int64)
    ineq_pool = np.array(rest[n_eq - len(must):], np.int64)
    others = np.array([i for i in range(m) if i not in set(cand) and i not in never], np.int64)
    free = set(int(i) for i in rng.choice(others, min(n_free, others.size), replace=False)) if others.size else set()
    B = len(counts)
    Q = np.empty((B, n)); L = np.empty((B, m)); U = np.empty((B, m))
    X = np.empty((B, n)); Y = np.empty((B, m)); act = np.empty((B, m), np.int64)
    for b, cnt in enumerate(counts):
        pick = rng.choice(ineq_pool, cnt, replace=False) if cnt else []
        Q[b], L[b], U[b], X[b], Y[b], act[b] = _plant_member(rng, P, A, eq, free, np.array(sorted(pick), np.int64))
    g = np.random.default_rng(seed + 4242)
    draw = lambda *s: g.standard_normal(s)
    inc = SimpleNamespace(gx=draw(B, n), gy=draw(B, m), dQ=draw(B, pq.NDIR, n), dL=draw(B, pq.NDIR, m),
                          dU=draw(B, pq.NDIR, m), dPx=draw(B, pq.NDIR, P.nnz), dAx=draw(B, pq.NDIR, A.nnz))
    return SimpleNamespace(name="common-" + name, n=n, m=m, B=B, P=P, A=A, Px_all=np.tile(P.data, (B, 1)),
                           Ax_all=np.tile(A.data, (B, 1)), Q=Q, L=L, U=U, x=X, y=Y, act=act, inc=inc, eq=eq, free=free,
                           settings={})


def _build(name):
    if name == "zero":       # mred = 0 in every member: NS = 32, S is the identity
        return _assemble(name, 31, 17, 37, 0, (0, 0, 0))
    if name == "ns_exact":   # mred = 32 = NS exactly beside mred = 1
        return _assemble(name, 32, 40, 56, 1, (31, 0, 12))
    if name == "no_p":       # variables without P entries, pinned by equality rows
        return _assemble(name, 35, 40, 56, 4, (10, 0, 20), must=NO_P, p_kw=dict(no_p=NO_P))
    if name == "rows":       # a dense row of A, a row of the full P and rows of A longer than 256, an empty column of A
        return _assemble(name, 36, 300, 310, 8, (112, 3), must=DENSE_A + (5, 7, 200), never=(EMPTY_COL,),
                         p_kw=dict(dense_row=0, no_p=(5, 7, 200)), a_kw=dict(dense_rows=DENSE_A, empty_col=EMPTY_COL))
    raise KeyError(name)


def _build_vertex(name):
    """mred = n: per variable exactly one active row, the equality rows fixed, the others row i or row i + n per member."""
    n, m, n_eq = 24, 48, 4
    rng = np.random.default_rng(33 if name == "vertex" else 34)
    P = pq._p_pattern(rng, n, empty=(name == "lp"))
    A = pq._a_pattern(rng, n, m)
    eq = np.sort(rng.choice(n, n_eq, replace=False)).astype(np.int64)          # rows eq[k] of variables eq[k]
    free = {int(r) + n for r in eq[:2]}                                      # their twins cannot be active: two are free
    B = 3
    Q = np.empty((B, n)); L = np.empty((B, m)); U = np.empty((B, m))
    X = np.empty((B, n)); Y = np.empty((B, m)); act = np.empty((B, m), np.int64)
    for b in range(B):
        pick = np.array(sorted(v + n * int(rng.integers(2)) for v in range(n) if v not in set(eq)), np.int64)
        Q[b], L[b], U[b], X[b], Y[b], act[b] = _plant_member(rng, P, A, eq, free, pick)
    g = np.random.default_rng(4242 + n)
    draw = lambda *s: g.standard_normal(s)
    inc = SimpleNamespace(gx=draw(B, n), gy=draw(B, m), dQ=draw(B, pq.NDIR, n), dL=draw(B, pq.NDIR, m),
                          dU=draw(B, pq.NDIR, m), dPx=draw(B, pq.NDIR, P.nnz), dAx=draw(B, pq.NDIR, A.nnz))
    return SimpleNamespace(name="common-" + name, n=n, m=m, B=B, P=P, A=A, Px_all=np.tile(P.data, (B, 1)),
                           Ax_all=np.tile(A.data, (B, 1)), Q=Q, L=L, U=U, x=X, y=Y, act=act, inc=inc, eq=eq, free=free,
                           settings={})


def case(name):
    """The case (built once, never modified)."""
    if name not in _cases:
        _cases[name] = _build_vertex(name) if name in ("vertex", "lp") else _build(name)
    return _cases[name]
