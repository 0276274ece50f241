"""GPU tests of the two direct linear-solve forms one KKT solve at a time, at their structural edges.

Dense-direct (res_kind 4, csrc/dense_direct.h, dense_direct_host.h) and block-direct (res_kind 3, k_blk_* / k_cap_* /
k_blk_apply_multi in engine_block_direct.h) are driven through the C shim: hipeng_create with no q, l, u, hipeng_kkt_solve, and the
three calls that form the inverse again (hipeng_upload_rho, hipeng_upload_matrices, hipeng_set_params with a new sigma).
Every case first asserts which form and which route inside it served the solve (hipeng_resident_info: [9] form, [3] dense
unknowns or blocks, [5] Cholesky route, [15] coupling rows kc or sparse-Schur variables nb2), then measures [x~; z~]
against the refined reference of tests/_kkt_reference.py:

  direct form in use, hipeng_kkt_solve (one refinement step on these forms):
      relative inf-norm forward error <= 10 x numpy's plain float64 error + 1e-14
  direct form in use, hipeng_kkt_solve_unrefined (one application of the inverse the ADMM loop iterates with):
      relative inf-norm forward error <= 10 x that of the float64 inverse of K (LAPACK) applied to the same rhs + 1e-14
  engine reports it fell back: ||rhs - K x~|| / ||rhs|| <= 10 x 1e-10 (the PCG stop of a solve outside the ADMM loop), both calls

Each solve prints its form, route and ratio (error / bar) for the record (pytest -s).

The refresh that drives the dense-direct engine off its direct form (cond 9e11, sigma 1e-10) asserts only that it left: the PCG
kernels it drops to reach no better than a relative residual of 0.3 there, far from the 1e-9 of the fallback bar; that leg is
left open."""
import numpy as np
import pytest
from scipy import sparse

from tests._direct_problems import _classes, bd_problem, dd_problem, spectrum_p
from tests._hipeng import Engine
from tests._kkt_reference import reduced_matrix

pytestmark = pytest.mark.gpu

SWEEP, CHOL = 0, 1


DD_ENV = dict(OSQP_AMD_RESIDENT=0, OSQP_AMD_DENSE_DIRECT=2)        # dense-direct whatever the size (block forms off)
BD_ENV = dict(OSQP_AMD_BLOCK_DIRECT=1)


# ---------------------------------------------------------------------------------------------------------------
# dense-direct problems
# ---------------------------------------------------------------------------------------------------------------
DD_SIZES = [1, 127, 128, 129, 1023, 1024, 1025, 1920, 1921]


@pytest.mark.parametrize("na", DD_SIZES)
def test_dense_direct_sizes(na):
    """Dense unknowns around the 128 padding, the small_only limit (1024) and the gemv / symv-tile switch (nap 2048).
    (One dense unknown: a variable with nine one-neighbour variables around it, which leave by the sparse Schur complement.)"""
    b2 = (1,) * 9 if na == 1 else ()
    Pu, A, rho = dd_problem(na, seed=na, row_len=40 if na >= 40 else na, nd=1 if na < 40 else None, b2_nbrs=b2)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        e.check(f"dd na={na}", 4)
        assert e.info()[3] == na and e.info()[15] == len(b2), e.info()
    finally:
        e.close()


@pytest.mark.parametrize("row_len", [0, 31, 32])
def test_dense_direct_row_lengths(row_len):
    """No dense rows, rows of exactly 31 entries (scattered) and of 32 (rows of R)."""
    Pu, A, rho = dd_problem(300, seed=row_len + 7, row_len=row_len, nd=0 if row_len == 0 else 6)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        e.check(f"dd rows of {row_len}", 4)
        assert e.info()[3] == 300
    finally:
        e.close()


@pytest.mark.parametrize("nbrs,in_b2", [((0, 8, 3), 3), ((9,), 0), ((8, 9, 0, 8), 3)])
def test_dense_direct_b2_neighbours(nbrs, in_b2):
    """Variables with 0 and 8 neighbours leave by the sparse Schur complement; one with 9 stays a dense unknown."""
    Pu, A, rho = dd_problem(200, seed=len(nbrs) * 11 + sum(nbrs), b2_nbrs=nbrs)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        e.check(f"dd B2 nbrs={nbrs}", 4)
        inf = e.info()
        assert inf[15] == in_b2 and inf[3] == 200 + len(nbrs) - in_b2, inf
    finally:
        e.close()


@pytest.mark.parametrize("pyy", [0.0, 0.7])
@pytest.mark.parametrize("shape", ["plain", "b2", "coupledP", "rows31"])
def test_dense_direct_with_eliminated_slacks(pyy, shape):
    """Slack-like variables eliminated by the engine (P_yy = 0 and > 0) next to B2 variables, a dense coupled P and
    31-entry rows: they must not count toward a row's length nor enter the dense set."""
    kw = dict(plain={}, b2=dict(b2_nbrs=(2, 8, 9)), coupledP=dict(Pcore=sparse.csc_matrix(spectrum_p(150, 100.0, 5))),
              rows31=dict(row_len=31, nd=4))[shape]
    Pu, A, rho = dd_problem(150, seed=int(pyy * 10) + len(shape), nslack=20, pyy=pyy, **kw)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        e.check(f"dd slacks pyy={pyy} {shape}", 4)
        assert e.elim() == 20
        inf = e.info()
        nb2 = 2 if shape == "b2" else 0
        assert inf[15] == nb2 and inf[3] == 150 + (1 if shape == "b2" else 0), inf
    finally:
        e.close()


def test_dense_direct_small_call_and_default_choice():
    """Without the forcing switch: at most 1024 dense unknowns take the dense-direct solve ahead of the resident PCG."""
    Pu, A, rho = dd_problem(1024, seed=3)
    e = Engine(Pu, A, rho, env=dict(OSQP_AMD_BLOCK_DIRECT=0))
    try:
        e.check("dd default 1024", 4)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# block-direct problems
# ---------------------------------------------------------------------------------------------------------------
BLOCKS = {"32": [32] * 6, "33": [33] * 5, "63": [63] * 4, "64": [64] * 4, "96": [96] * 3, "127": [127] * 2, "128": [128] * 2,
          "mixed": [32, 128, 33, 63, 96, 64, 127, 40]}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_direct_block_sizes(name):
    """Plain form (single-entry rows only) at block sizes 32 .. 128, around the pitch rule and a mixed tiling."""
    blocks = BLOCKS[name]
    Pu, A, rho = bd_problem(blocks, seed=len(name) + blocks[0])
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        e.check(f"bd blocks {name}", 3)
        inf = e.info()
        assert inf[3] == len(blocks) and inf[15] == 0, inf
    finally:
        e.close()


def test_block_direct_explicit_zeros_in_block():
    """A block whose stored upper triangle is a third explicit zeros still passes the density rule and is inverted whole."""
    Pu, A, rho = bd_problem([64, 96, 64], seed=9, zeros_in=1)
    assert (Pu.data == 0.0).sum() > 1000
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        e.check("bd explicit zeros", 3)
        assert e.info()[3] == 3
    finally:
        e.close()


@pytest.mark.parametrize("kc", [1, 15, 16, 17, 32, 33, 512])
def test_block_direct_coupled_rows(kc):
    """Coupling rows as the Woodbury term, in 16-column groups of k_blk_apply_multi / k_cpl_dot, up to CPL_MAX."""
    Pu, A, rho = bd_problem([64, 128, 96, 64, 128, 32, 100], seed=kc, kc=kc)
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        e.check(f"bd kc={kc}", 3)
        assert e.info()[15] == kc
    finally:
        e.close()


def test_block_direct_not_chosen_above_cpl_max():
    """513 coupling rows: not the block-direct form; the dense-direct small call takes the 612 unknowns instead."""
    Pu, A, rho = bd_problem([64, 128, 96, 64, 128, 32, 100], seed=513, kc=513)
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        inf = e.info()
        assert inf[9] == 4 and inf[3] == 612, inf
        e.check("bd kc=513", 4)
    finally:
        e.close()


@pytest.mark.parametrize("nhuge,form_kc", [(1, 0), (4, 0), (5, 5)])
def test_block_direct_huge_rows(nhuge, form_kc):
    """Huge rows (>= 8192 entries): up to 4 folded into the plain form; 5 are not folded and enter as coupling rows."""
    Pu, A, rho = bd_problem([128] * 64, seed=nhuge, nhuge=nhuge)
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        inf = e.info()
        assert inf[9] == 3 and inf[3] == 64 and inf[15] == form_kc, inf
        e.check(f"bd huge={nhuge}", 3, nrhs=2)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------------------
CONDS = [1e1, 1e4, 1e5, 1e6, 1e8]


def _cond(e):
    return float(np.linalg.cond(reduced_matrix(e.Pu, e.A, e.sigma, e.rho)))


@pytest.mark.parametrize("cond", CONDS)
def test_dense_direct_conditioning(cond):
    Pu, A, rho = dd_problem(256, seed=int(np.log10(cond)), Pcore=sparse.csc_matrix(spectrum_p(256, cond, 1)), nshort=20, nd=2, a_scale=0.3)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        c = _cond(e)
        assert cond / 30 <= c <= cond * 30, c
        inf = e.info()
        print(f"[direct-edges] dd cond {c:.1e}: form {inf[9]} route {inf[5]}")
        e.check(f"dd cond {c:.0e}", 4, CHOL if cond >= 1e6 else None)     # (the sweeps' inverse fails its probe checks from cond ~1e6 on)     # (the sweep inverse fails its probe check from cond ~1e6 on)
    finally:
        e.close()


@pytest.mark.parametrize("cond", CONDS)
def test_block_direct_conditioning(cond):
    Pu, A, rho = bd_problem([64] * 4, seed=int(np.log10(cond)) + 40, cond=cond, kc=8, single=True)
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        c = _cond(e)
        print(f"[direct-edges] bd cond {c:.1e}: form {e.info()[9]}")      # (the 64-wide blocks pass their check up to cond 2e7)
        e.check(f"bd cond {c:.0e}", 3)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# refresh paths on one live engine
# ---------------------------------------------------------------------------------------------------------------
def test_dense_direct_refresh_paths():
    Pu, A, rho = dd_problem(200, seed=21, b2_nbrs=(3, 5), nslack=10, pyy=0.3)
    e = Engine(Pu, A, rho, env=DD_ENV)
    try:
        e.check("dd refresh: start", 4)
        # (the sweeps' inverse of this one is 100x less accurate than a float64 inverse; its known-solution probe sends it to the
        # Cholesky route)
        e.set_rho(rho * 10.0); e.check("dd refresh: rho x10", 4, CHOL)
        e.set_rho(rho / 10.0); e.check("dd refresh: rho /10", 4)
        e.set_rho(_classes(e.m, np.random.default_rng(5), eq=0.5, loose=0.3)); e.check("dd refresh: classes", 4)
        e.set_sigma(1e-3); e.check("dd refresh: sigma", 4)
        # new values, same pattern: the core of P scaled toward singular, then back; then far enough (sigma 1e-10 too) that
        # the Cholesky inverse fails its check and the engine leaves the dense-direct form for the PCG kernels for good
        for s, tag, route in ((1e-3, "P x1e-3", None), (1e-7, "P x1e-7", CHOL), (1.0, "P x1", None)):
            coo = Pu.tocoo()
            scale = np.where(coo.col < 200, s, 1.0)
            Pn = sparse.csc_matrix((coo.data * scale, (coo.row, coo.col)), shape=Pu.shape)
            An = A.copy(); An.data = An.data * (1.0 + 0.1 * np.sin(np.arange(An.nnz)))
            e.set_matrices(Pn, An)
            inf = e.info()
            print(f"[direct-edges] dd refresh {tag}: cond {_cond(e):.1e} form {inf[9]} route {inf[5]}")
            e.check(f"dd refresh: {tag}", 4, route)
        e.set_sigma(1e-10)
        coo = Pu.tocoo()
        e.set_matrices(sparse.csc_matrix((coo.data * np.where(coo.col < 200, 1e-9, 1.0), (coo.row, coo.col)), shape=Pu.shape), A)
        inf = e.info()
        print(f"[direct-edges] dd refresh P x1e-9 sigma 1e-10: cond {_cond(e):.1e} form {inf[9]} route {inf[5]}")
        assert inf[9] == 0, inf          # (its accuracy: see the note in the module docstring)
    finally:
        e.close()


def test_block_direct_refresh_paths():
    Pu, A, rho = bd_problem([64, 96, 128, 64], seed=31, kc=20)
    e = Engine(Pu, A, rho, env=BD_ENV)
    try:
        e.check("bd refresh: start", 3)
        e.set_rho(rho * 10.0); e.check("bd refresh: rho x10", 3)
        e.set_rho(rho / 10.0); e.check("bd refresh: rho /10", 3)
        e.set_rho(_classes(e.m, np.random.default_rng(6), eq=0.5, loose=0.3)); e.check("bd refresh: classes", 3)
        e.set_sigma(1e-3); e.check("bd refresh: sigma", 3)
        for s, tag in ((1e-3, "P x1e-3"), (1e-7, "P x1e-7"), (1.0, "P x1")):
            An = A.copy(); An.data = An.data * (1.0 + 0.1 * np.cos(np.arange(An.nnz)))
            e.set_matrices(Pu * s, An)
            inf = e.info()
            print(f"[direct-edges] bd refresh {tag}: cond {_cond(e):.1e} form {inf[9]}")
            e.check(f"bd refresh: {tag}", 3)
    finally:
        e.close()


def test_two_dense_direct_engines_interleaved():
    """Engines of nap 1920 (k_dd_gemv, 15 KiB of LDS) and 128: the smaller one is created second, then both are refreshed and
    solved in turn.  Each stays within its own bar."""
    big = Engine(*dd_problem(1920, seed=41), env=DD_ENV)
    small = Engine(*dd_problem(100, seed=42), env=DD_ENV)
    try:
        for k in range(2):
            big.check(f"two engines: nap 1920 #{k}", 4, seed=k)
            small.check(f"two engines: nap 128 #{k}", 4, seed=k)
            big.set_rho(big.rho * 3.0)
            small.set_rho(small.rho * 3.0)
        assert big.info()[3] == 1920 and small.info()[3] == 100
    finally:
        big.close()
        small.close()
