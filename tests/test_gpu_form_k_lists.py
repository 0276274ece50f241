"""k_form_K_lists (engine_pcg_resident.h): the values of the resident K summed from the contribution lists of the set-up, against k_form_K
(OSQP_AMD_FORM_K_LISTS=0), which merges the patterns on the device each time.  Same operands, same association, same order of
the terms: the two must agree to the bit (hipeng_resident_dump), whatever rho, sigma and the matrices' values are, with
eliminated variables, at the turns of either kernel's loops.  Then whole solves: lists against no lists (same bits), against the
oracle (the bars of test_gpu_resident.test_resident_modes_match_oracle).

Agreement of the two kernels is not yet the documented value: a term dropped, doubled or taken from the wrong slot in both would
pass.  So every state is also compared, bit for bit, with tests/_form_k_reference.replay -- the documented sequence of float64
operations repeated by numpy from the engine's own (Pu, A, sigma, rho or rhoe), which knows neither kernel nor the lists -- for
both engines, on cases cut for the turns of k_form_K_lists's own loops (tests/_form_k_cases.py: col66 .. col131, pair2 / pair3,
shared70x67, krow300_tail), with a long list under elimination and through a whole solve."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from tests import _form_k_cases as FC
from tests import _form_k_reference as FR
from tests._hipeng import Engine
from tests.test_gpu_resident import _env, _info, _qp, _rel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("pcg_paths")]
ENV = dict(OSQP_AMD_DENSE_DIRECT=0, OSQP_AMD_RESIDENT_MIN_N=1)
OFF = dict(OSQP_AMD_FORM_K_LISTS=0)


def _form_k_info(handle):
    """hipeng_form_k_info: [0] lists in use, [1] terms, [2] bytes of the lists, [3] budget in bytes"""
    import osqp_amd
    f = osqp_amd.lib().hipeng_form_k_info
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 4)()
    assert f(handle, out) == 0
    return list(out)


def _dump(handle, nnz):
    import osqp_amd
    f = osqp_amd.lib().hipeng_resident_dump
    f.restype, f.argtypes = C.c_longlong, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    row = np.zeros(nnz, dtype=np.int32); col = np.zeros(nnz, dtype=np.int32); val = np.zeros(nnz)
    assert f(handle, row.ctypes.data, col.ctypes.data, val.ctypes.data, nnz) == nnz
    return row, col, val


def _same_K(tag, h0, h1, nnz):
    """The two engines hold the same K, bit for bit (np.array_equal, and the sign of a zero with it)."""
    r0, c0, v0 = _dump(h0, nnz)
    r1, c1, v1 = _dump(h1, nnz)
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1), tag
    diff = int((v0.view(np.int64) != v1.view(np.int64)).sum())
    print(f"[form-k-lists] {tag}: {nnz} entries of K, {diff} differ, max |K| {np.abs(v0).max():.3e}")
    assert np.isfinite(v0).all() and np.abs(v0).max() > 0.0, tag
    assert np.array_equal(v0, v1) and diff == 0, tag
    return v0


def _pattern(handle, nnz):
    """The dumped triplets (row, column, value) in the plan's order: row by row, columns ascending."""
    row, col, val = _dump(handle, nnz)
    order = np.lexsort((col, row))
    return row[order].astype(np.int64), col[order].astype(np.int64), val[order]


def _gone(e):
    """The variables the engine eliminated (build_elim's rule on the host, checked against what the engine reports), as a list."""
    gone, taken = FR.eliminated(e.Pu, e.A)
    assert e.elim() == len(gone), (e.elim(), len(gone))
    assert [i for i in range(e.m) if e.row_eliminated(i)] == taken
    return gone


def _is_replay(tag, engines, nnz, gone=()):
    """Every engine holds, bit for bit, the K that the documented sequence gives on its own (Pu, A, sigma, rho) -- rhoe and unit
    diagonals where variables are eliminated.  Returns the lengths of the lists (entries in the plan's order)."""
    for which, e in engines:
        row, col, val = _pattern(e.h, nnz)
        Kptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=e.n))])
        w = e.elim_peek("rhoe") if len(gone) else e.rho
        ref, _, _, cnt = FR.replay(e.Pu, e.A, e.sigma, w, Kptr, col, gone=gone)
        diff = int((val.view(np.int64) != ref.view(np.int64)).sum())
        print(f"[form-k-lists] {tag} ({which}): {nnz} entries of K, {diff} differ from the replay, longest list {int(cnt.max()) if len(cnt) else 0}")
        assert np.array_equal(val.view(np.int64), ref.view(np.int64)) and diff == 0, (tag, which, diff)
    return Kptr, col, cnt


@pytest.mark.parametrize("name", FC.GPU_CASES)
def test_lists_give_the_bits_of_the_merge(name):
    P, A = FC.case(name)
    n, m = P.shape[0], A.shape[0]
    Pu = sparse.triu(P, format="csc")
    rng = np.random.default_rng(len(name))
    rho = np.full(m, 0.1)
    e0, e1 = Engine(Pu, A, rho, env={**ENV, **OFF}), Engine(Pu, A, rho, env=ENV)
    try:
        i0, i1 = e0.info(), e1.info()
        assert i0[9] == 1 and i1[9] == 1 and i0[1] and i1[1], (name, i0, i1)          # both on k_pcg_resident
        assert i0[2:5] == i1[2:5]
        f0, f1 = _form_k_info(e0.h), _form_k_info(e1.h)
        terms = int((np.diff(sparse.csr_matrix(A).indptr).astype(np.int64) ** 2).sum())
        assert f0[0] == 0 and f0[2] == 0 and f1[0] == 1 and f0[1] == f1[1] == terms, (f0, f1)
        assert f1[2] == 8 * terms + 4 * (i1[4] + 1) and f1[3] == 128 << 20, f1
        nnz = int(i1[4])
        if name == "krow300":
            row = _dump(e1.h, nnz)[0]
            assert np.bincount(row).max() > 256
        both = (("merge", e0), ("lists", e1))
        gone = _gone(e1)
        assert _gone(e0) == gone
        seen = [_same_K(f"{name} set-up", e0.h, e1.h, nnz)]
        Kptr, Kcol, lens = _is_replay(f"{name} set-up", both, nnz, gone)
        FC.check_premise(name, Kptr, Kcol, lens)                 # (a list of 67 terms or more where the case is there for one)
        if m:
            # rho over six decades, then equality rows (1e3 rho) among the others
            for tag, r in (("rho 1e-3..1e3", 10.0 ** rng.uniform(-3.0, 3.0, m)), ("equality rows", np.where(np.arange(m) % 3 == 0, 100.0, 0.1))):
                e0.set_rho(r); e1.set_rho(r)
                seen.append(_same_K(f"{name} {tag}", e0.h, e1.h, nnz))
                _is_replay(f"{name} {tag}", both, nnz, gone)
        # new values of P and of A on the same patterns
        Pu2, A2 = Pu.copy(), sparse.csc_matrix(A).copy()
        Pu2.data = Pu.data * (1.0 + 0.2 * rng.standard_normal(Pu.nnz)); A2.data = A2.data * (1.0 + 0.2 * rng.standard_normal(A2.nnz))
        e0.set_matrices(Pu2, A2); e1.set_matrices(Pu2, A2)
        seen.append(_same_K(f"{name} new P, A", e0.h, e1.h, nnz))
        _is_replay(f"{name} new P, A", both, nnz, gone)
        e0.set_sigma(0.03); e1.set_sigma(0.03)                   # (large against 1e-6: it moves the bits of every diagonal entry)
        seen.append(_same_K(f"{name} sigma 0.03", e0.h, e1.h, nnz))
        _is_replay(f"{name} sigma 0.03", both, nnz, gone)
        for a, b in zip(seen[:-1], seen[1:]):
            assert not np.array_equal(a, b)                    # every update reached K
        # ... and it is the K of the formula (the bar of test_gpu_pcg_edges for hipeng_resident_dump), symmetric to the bit.  Where
        # the engine eliminated a variable (a column of A with one entry and no coupling in P) K is that of the reduced system,
        # which tests/test_gpu_elim_edges.py checks; here the agreement of the two kernels above is the point.
        K = e1.resident_dump()
        assert np.array_equal(K, K.T)
        assert e0.elim() == e1.elim()
        if e1.elim() == 0:
            Pf = (Pu2 + sparse.triu(Pu2, 1).T).toarray(); Ad = A2.toarray()
            Kref = Pf + e1.sigma * np.eye(n) + Ad.T @ (e1.rho[:, None] * Ad)
            assert np.abs(K - Kref).max() <= 1e-13 * np.abs(Kref).max()
    finally:
        e0.close(); e1.close()


def test_lists_with_eliminated_variables(gpu_lib):
    """The Lasso of tests/test_gpu_elim.py (n = 600, its 300 residual variables eliminated): their rows and columns of K hold a
    unit diagonal and the rows' weights are the effective ones (rhoe) in both kernels."""
    import osqp_amd
    from osqp_amd.problems import lasso_qp
    from tests.test_gpu_elim import _elim_count
    pb = lasso_qp(150, 300, density=0.15, seed=3)
    data = {k: pb[k] for k in "PqAlu"}
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50)
    with _env(OSQP_AMD_FORM_K_LISTS=0):
        s0 = osqp_amd.OSQP().setup(**data, **kw)
    s1 = osqp_amd.OSQP().setup(**data, **kw)
    assert _elim_count(s0) == 300 and _elim_count(s1) == 300
    i0, i1 = _info(s0), _info(s1)
    assert i0["form"] == 1 and i1["form"] == 1 and i0["in_use"] and i1["in_use"] and i0["nnzK"] == i1["nnzK"]
    assert _form_k_info(s0.engine())[0] == 0 and _form_k_info(s1.engine())[0] == 1
    nnz = int(i1["nnzK"])
    v = _same_K("lasso set-up", s0.engine(), s1.engine(), nnz)
    r, c, _ = _dump(s1.engine(), nnz)
    assert int(((r == c) & (v == 1.0)).sum()) >= 300            # the eliminated variables' unit diagonals
    for s in (s0, s1): s.update_rho(0.3)
    _same_K("lasso update_rho", s0.engine(), s1.engine(), nnz)
    A = sparse.csc_matrix(data["A"]); A.sort_indices()
    Ax = A.data * (1.0 + 0.01 * np.random.default_rng(5).standard_normal(A.nnz))
    for s in (s0, s1): assert s.update(Ax=Ax) == 0
    _same_K("lasso update A", s0.engine(), s1.engine(), nnz)
    r0, r1 = s0.solve(), s1.solve()
    assert r0.info.status == r1.info.status == "solved" and r0.info.iter == r1.info.iter
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.y, r1.y)
    assert _info(s1)["gave_up"] == 0 and _info(s0)["gave_up"] == 0


def test_a_solve_with_lists_without_them_and_against_the_oracle(gpu_lib, oracle_mod):
    """A QP with equality rows and rho updates in the solve (each forms K again): with lists, with OSQP_AMD_FORM_K_LISTS=0 and
    with a budget of 0 MB (lists reported as not in use) the iterates are the same bits; against the oracle the bars of
    test_resident_modes_match_oracle."""
    import osqp_amd
    pb = _qp(900, 700, 11, eq=200)
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25)
    s1 = osqp_amd.OSQP().setup(**pb, **kw)
    with _env(OSQP_AMD_FORM_K_LISTS=0):
        s0 = osqp_amd.OSQP().setup(**pb, **kw)
    with _env(OSQP_AMD_FORM_K_LIST_MB=0):
        sb = osqp_amd.OSQP().setup(**pb, **kw)
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    f1, f0, fb = _form_k_info(s1.engine()), _form_k_info(s0.engine()), _form_k_info(sb.engine())
    assert f1[0] == 1 and f1[2] > 0 and f0[0] == 0 and fb[0] == 0 and fb[2] == 0 and fb[3] == 0 and f1[1] == f0[1] == fb[1] > 0, (f1, f0, fb)
    assert all(_info(s)["in_use"] and _info(s)["form"] == 1 for s in (s1, s0, sb))
    r1, r0, rb, ro = s1.solve(), s0.solve(), sb.solve(), so.solve()
    assert r1.info.status == ro.info.status == "solved"
    assert r1.info.iter == ro.info.iter and r1.info.rho_updates == ro.info.rho_updates and r1.info.rho_updates > 0
    assert _rel(r1.x, ro.x) < 1e-6 and _rel(r1.y, ro.y) < 1e-6
    assert abs(r1.info.obj_val - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val))
    for r in (r0, rb):
        assert r.info.iter == r1.info.iter and np.array_equal(r.x, r1.x) and np.array_equal(r.y, r1.y)
    for s in (s1, s0, sb):
        inf = _info(s)
        assert inf["in_use"] and inf["gave_up"] == 0, inf


def test_a_long_list_under_elimination():
    """A small dense Lasso at the engine's level: n = 96, its 80 residual variables eliminated, and every feature's column of A has
    the 80 data rows and two more -- lists of 80 and 82 terms whose weights are the effective ones (rhoe) and whose neighbours in
    the row are unit or zero entries of eliminated variables.  lists == merge == replay at set-up, after new rho, new matrices."""
    from osqp_amd.problems import lasso_qp
    pb = lasso_qp(n_feat=8, m_data=80, density=1.0, seed=3)
    Pu, A = sparse.csc_matrix(pb["P"]), sparse.csc_matrix(pb["A"])
    n, m = Pu.shape[0], A.shape[0]
    assert n == 96 and np.diff(A.indptr)[:8].min() >= 80
    rng = np.random.default_rng(8)
    rho = np.where(pb["l"] == pb["u"], 100.0, 0.1)
    e0, e1 = Engine(Pu, A, rho, env={**ENV, **OFF}), Engine(Pu, A, rho, env=ENV)
    try:
        i0, i1 = e0.info(), e1.info()
        assert i0[9] == 1 and i1[9] == 1 and i0[1] and i1[1], (i0, i1)
        assert _form_k_info(e0.h)[0] == 0 and _form_k_info(e1.h)[0] == 1
        nnz = int(i1[4])
        both = (("merge", e0), ("lists", e1))
        gone = _gone(e1)
        assert _gone(e0) == gone and len(gone) == 80 and gone == list(range(8, 88))
        v = _same_K("lasso96 set-up", e0.h, e1.h, nnz)
        Kptr, Kcol, lens = _is_replay("lasso96 set-up", both, nnz, gone)
        assert lens.max() == 82 and int((lens >= 67).sum()) == 64             # the 8 x 8 block of the features
        rows = np.repeat(np.arange(n), np.diff(Kptr))
        v = _pattern(e1.h, nnz)[2]
        assert int(((rows == Kcol) & (v == 1.0)).sum()) == 80 and (v[(np.isin(rows, gone) | np.isin(Kcol, gone)) & (rows != Kcol)] == 0.0).all()
        r = 10.0 ** rng.uniform(-3.0, 3.0, m)
        e0.set_rho(r); e1.set_rho(r)
        v2 = _same_K("lasso96 rho 1e-3..1e3", e0.h, e1.h, nnz)
        _is_replay("lasso96 rho 1e-3..1e3", both, nnz, gone)
        Pu2, A2 = Pu.copy(), A.copy()
        Pu2.data = Pu.data * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, Pu.nnz)); A2.data = A.data * (1.0 + 0.2 * rng.standard_normal(A.nnz))
        e0.set_matrices(Pu2, A2); e1.set_matrices(Pu2, A2)
        v3 = _same_K("lasso96 new P, A", e0.h, e1.h, nnz)
        _is_replay("lasso96 new P, A", both, nnz, gone)
        assert not np.array_equal(v, v2) and not np.array_equal(v2, v3)
    finally:
        e0.close(); e1.close()


def _qp_long_column(n, m, seed, rows, eq):
    """The recipe of test_gpu_resident._qp with one column of A holding `rows` entries (planted before the bounds are drawn)."""
    rng = np.random.default_rng(seed)
    A = sparse.random(m, n, density=0.02, random_state=seed, data_rvs=rng.standard_normal, format="lil")
    for k in range(min(m, n)): A[k, k] = A[k, k] + 1.0
    col = n // 3
    A[:, col] = 0.0
    for r in np.sort(rng.choice(m, rows, replace=False)): A[r, col] = rng.standard_normal()
    A = sparse.csc_matrix(A); A.eliminate_zeros(); A.sort_indices()
    B = sparse.random(n, n, density=0.02, random_state=seed + 1, data_rvs=rng.standard_normal, format="csc")
    P = (B @ B.T + 0.05 * sparse.eye(n)).tocsc()
    q = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    l = A @ x0 - rng.uniform(0.1, 1, m); u = A @ x0 + rng.uniform(0.1, 1, m)
    l[:eq] = u[:eq]
    return dict(P=P, q=q, A=A, l=l, u=u), col


def test_a_solve_over_a_long_list(gpu_lib, oracle_mod, monkeypatch):
    """A whole solve whose K has a 131-term list (Ruiz-scaled values, rho updates that form K again): with lists, with
    OSQP_AMD_FORM_K_LISTS=0 and with a budget of 0 MB the same iterations and the same bits of x and y; against the oracle the
    bars of test_resident_modes_match_oracle."""
    import osqp_amd
    for k, v in ENV.items():
        monkeypatch.setenv(k, str(v))
    pb, col = _qp_long_column(300, 340, 21, 131, eq=60)
    assert np.diff(pb["A"].indptr)[col] == 131
    kw = dict(eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25)
    s1 = osqp_amd.OSQP().setup(**pb, **kw)
    with _env(OSQP_AMD_FORM_K_LISTS=0):
        s0 = osqp_amd.OSQP().setup(**pb, **kw)
    with _env(OSQP_AMD_FORM_K_LIST_MB=0):
        sb = osqp_amd.OSQP().setup(**pb, **kw)
    so = oracle_mod.OracleOSQP().setup(**pb, **kw)
    f1, f0, fb = _form_k_info(s1.engine()), _form_k_info(s0.engine()), _form_k_info(sb.engine())
    assert f1[0] == 1 and f1[2] > 0 and f0[0] == 0 and fb[0] == 0 and f1[1] == f0[1] == fb[1] > 0, (f1, f0, fb)
    assert all(_info(s)["in_use"] and _info(s)["form"] == 1 for s in (s1, s0, sb))
    # the premise, from the pattern the engine holds: one list of 131 terms, on the diagonal of the planted column
    nnz = int(_info(s1)["nnzK"])
    row, colK, _ = _pattern(s1.engine(), nnz)
    Kptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=300))])
    lens = FR.replay(pb["P"], pb["A"], 0.0, np.ones(340), Kptr, colK)[3]
    assert lens.max() == 131 and lens[(row == col) & (colK == col)] == 131 and int(lens.sum()) == f1[1]
    assert _same_K("long column before the solve", s0.engine(), s1.engine(), nnz) is not None
    r1, r0, rb, ro = s1.solve(), s0.solve(), sb.solve(), so.solve()
    differ = sum(int((a.view(np.int64) != b.view(np.int64)).sum()) for r in (r0, rb) for a, b in ((r.x, r1.x), (r.y, r1.y)))
    print(f"[form-k-lists] long column solve: {nnz} entries of K, {differ} elements of x, y differ among lists / merge / no budget, longest list {int(lens.max())}, "
          f"{r1.info.iter} iterations, {r1.info.rho_updates} rho updates")
    assert r1.info.status == ro.info.status == "solved"
    assert r1.info.iter == ro.info.iter and r1.info.rho_updates == ro.info.rho_updates and r1.info.rho_updates > 0
    assert _rel(r1.x, ro.x) < 1e-6 and _rel(r1.y, ro.y) < 1e-6
    assert abs(r1.info.obj_val - ro.info.obj_val) <= 1e-8 * max(1.0, abs(ro.info.obj_val))
    for r in (r0, rb):
        assert r.info.iter == r1.info.iter and np.array_equal(r.x, r1.x) and np.array_equal(r.y, r1.y)
    _same_K("long column after the solve", s0.engine(), s1.engine(), nnz)
    for s in (s1, s0, sb):
        inf = _info(s)
        assert inf["in_use"] and inf["gave_up"] == 0, inf
