"""CPU tests of tests/_dense_reference.py, the references and bars that tests/test_gpu_dense_kernels.py holds the dense-direct
GEMM kernels and inversion routes to (no library, no device):

  * each restatement of a route inverts: on every case the Cholesky restatement is within 10 x numpy's own inv of the truth; the
    sweep restatement's ratio to numpy's is printed (its error grows like cond^2 eps: that is the route, not a defect);
  * the GEMM bound holds for a float64 numpy product of every case, and the masks leave exactly the named tiles;
  * every planted one-place defect misses its bar by more than 10 x;
  * no bar is so wide that an O(1e-6) relative error would pass: bar <= 1e-9 max|result| for every case."""
import numpy as np
import pytest

from tests import _dense_reference as DR


@pytest.mark.parametrize("name", list(DR.GEMM_CASES))
def test_gemm_bound_holds_for_a_float64_product(name):
    c = DR.GEMM_CASES[name]
    ref, untouched, bound = DR.gemm_reference(c)
    worst, changed = DR.gemm_miss(DR.gemm_model(c), c, ref, untouched, bound)
    print(f"[dense-ref] gemm {name}: float64 numpy err/bound {worst:.3f}, {int((~untouched).sum())} entries written")
    assert changed == 0 and worst <= 1.0
    # written: the unmasked tiles inside M x N, nothing else
    M, N = c["M"], c["N"]
    assert not (~untouched)[M:].any() and not (~untouched)[:, N:].any()
    assert np.all(np.isfinite(ref[~untouched].astype(float)))
    # the bar is sharp
    assert bound[~untouched].max() <= 1e-9 * np.abs(ref[~untouched]).max()
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            assert np.all((np.abs(v) >= 0.5) & (np.abs(v) <= 2.0) | np.isnan(v)), k


def test_gemm_masks_name_the_tiles_of_the_issue():
    """sweep_kb1: only tiles (0,0), (2,0), (2,2) change; chol_kb0: (1,1), (2,1), (2,2); kmode2: the lower tiles; an unmasked case
    against the plain formula."""
    def tiles(name):
        _, untouched, _ = DR.gemm_reference(DR.GEMM_CASES[name])
        t = ~untouched
        got = {(i, j) for i in range(t.shape[0] // 128) for j in range(t.shape[1] // 128) if t[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128].any()}
        assert all(t[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128].all() for i, j in got)
        return got
    assert tiles("sweep_kb1") == {(0, 0), (2, 0), (2, 2)}
    assert tiles("chol_kb0") == {(1, 1), (2, 1), (2, 2)}
    assert tiles("kmode2") == {(0, 0), (1, 0), (1, 1)}
    c = DR.GEMM_CASES["k33"]
    ref, _, _ = DR.gemm_reference(c)
    plain = (c["T"].astype(DR.LD).T * c["w"].astype(DR.LD)) @ c["B"].astype(DR.LD)
    assert np.abs(ref - plain).max() <= 1e-17 * np.abs(plain).max()
    c = DR.GEMM_CASES["kmode2"]                     # k from the row tile on
    ref, _, _ = DR.gemm_reference(c)
    plain = c["T"][128:, 128:].astype(DR.LD).T @ c["B"][128:, :128].astype(DR.LD)
    assert np.abs(ref[128:, :128] - plain).max() <= 1e-17 * np.abs(plain).max()


@pytest.mark.parametrize("defect", list(DR.GEMM_DEFECTS))
def test_gemm_bound_sees_each_planted_defect(defect):
    for name in DR.GEMM_DEFECTS[defect]:
        c = DR.GEMM_CASES[name]
        ref, untouched, bound = DR.gemm_reference(c)
        worst, changed = DR.gemm_miss(DR.gemm_model(c, defect), c, ref, untouched, bound)
        print(f"[dense-ref] gemm {name}: {defect}: err/bound {worst:.2e}, {changed} untouched entries changed")
        assert worst > 10.0, (name, defect, worst)


@pytest.mark.parametrize("name", DR.INVERT_NAMES)
def test_restatements_invert_and_bars_are_sharp(name):
    c = DR.invert_case(name)
    n, A = c["n"], c["A"]
    ev = np.linalg.eigvalsh(A)
    hi = 1e3 if name == "spread384" else 10.0
    assert abs(ev[0] - 1.0) < 1e-9 and abs(ev[-1] - hi) < 1e-9 * hi
    # the truth is one: its own residual (long double roundings times cond) is under 1 % of the smallest bar
    assert np.abs(c["resid0"]).max() <= 0.01 * min(c[r]["bar"][1] for r in (DR.SWEEP, DR.CHOL))
    npe = c["numpy"]
    for route, tag in ((DR.CHOL, "cholesky"), (DR.SWEEP, "sweep")):
        e, bar = c[route]["err"], c[route]["bar"]
        print(f"[dense-ref] {name} {tag}: restatement |X - truth| {e[0]:.2e} (numpy {npe[0]:.2e}, ratio {e[0] / npe[0]:.2f}), "
              f"|XA - I| {e[1]:.2e} (numpy {npe[1]:.2e}, ratio {e[1] / npe[1]:.2f}); bars {bar[0]:.2e} {bar[1]:.2e}")
        if route == DR.CHOL:
            assert e[0] <= 10.0 * npe[0] and e[1] <= 10.0 * npe[1]
        assert bar[0] <= 1e-9 * c["amax"] and bar[1] <= 1e-9
    if name == "tail256":
        assert np.array_equal(A[129:, 129:], np.eye(127)) and not A[129:, :129].any()


@pytest.mark.parametrize("name", ["n256", "n768", "spread384"])
@pytest.mark.parametrize("defect", DR.SWEEP_DEFECTS)
def test_inversion_bar_sees_each_planted_defect(name, defect):
    c = DR.invert_case(name)
    e = DR.invert_errors(c, DR.sweep_reference(c["A"], defect))
    bar = c[DR.SWEEP]["bar"]
    print(f"[dense-ref] {name}: {defect}: |X - truth| {e[0] / bar[0]:.2e} x bar, |XA - I| {e[1] / bar[1]:.2e} x bar")
    assert e[0] > 10.0 * bar[0] and e[1] > 10.0 * bar[1]


def test_verdict_cases_are_what_they_claim():
    for tag, A, verdict in DR.verdict_cases():
        assert A.shape == (256, 256) and np.array_equal(A, A.T)
        assert (np.linalg.eigvalsh(A)[0] <= 0.0) == bool(verdict), tag
        if tag.startswith("coupling"):
            assert np.all(np.diag(A) > 0.0)
