"""Host test of tests/_resident_startup.py, the float64 replay of the start-up sum of k_pcg_resident that
tests/test_gpu_resident_startup.py compares the launch's tol2 with, against a long-double sum of the same partials.

Bound.  A lane adds ceil(gridM / 64) partials (the first to 0.0: exact), wave_sum adds six levels more: no partial passes through more
than ceil(gridM / 64) + 5 rounded additions, each with a relative error of at most 2^-53 on an intermediate sum of magnitude at most
(1 + small) * sum |part|.  The issue's bar, (ceil(gridM / 64) + 7) * 2^-53 * sum |part|, leaves two units for the second-order terms
and for the rounding of the long-double reference.  tol2 = max((eps_rel * eps_rel) * bb, eps_abs^2) adds two roundings, of eps_rel^2
and of the product.

gridM: 1 (one lane, one partial), 63 / 64 / 65 (a wavefront not full, full, one lane with a second partial), 129 (three rounds, the
last of one lane) and the cap of 1024 (sixteen partials in every lane)."""
import math

import numpy as np
import pytest

from tests import _resident_startup as S

LD = np.longdouble
SIZES = (1, 63, 64, 65, 129, 1024)
EPS_REL, EPS_ABS = 1e-12, 1e-15


def _parts(g, kind):
    rng = np.random.default_rng(7000 + g)
    if kind == "squares":                                     # what k_pcg_init leaves: sums of squares, of mixed magnitudes
        return rng.standard_normal(g) ** 2 * 10.0 ** rng.uniform(-6, 6, g)
    return rng.standard_normal(g) * 10.0 ** rng.uniform(-6, 6, g)      # mixed signs: cancellation inside the bar's sum |part|


def _bar(part):
    return (math.ceil(len(part) / 64) + 7) * 2.0 ** -53 * float(np.abs(part).astype(LD).sum())


@pytest.mark.parametrize("kind", ["squares", "signed"])
@pytest.mark.parametrize("g", SIZES)
def test_replay_against_long_double(g, kind):
    part = _parts(g, kind)
    ref = part.astype(LD).sum()
    got = S.start_sum(part)
    err = abs(float(LD(got) - ref))
    print(f"[resident-startup] gridM {g} {kind}: err {err:.3e} bar {_bar(part):.3e}")
    assert err <= _bar(part), (g, kind, err, _bar(part))
    # tol2: two more roundings
    t_ref = max(LD(EPS_REL) * LD(EPS_REL) * ref, LD(EPS_ABS) * LD(EPS_ABS))
    t_got = S.tol2(part, EPS_REL, EPS_ABS)
    t_bar = EPS_REL * EPS_REL * _bar(part) * (1.0 + 2.0 ** -50) + 2.0 * 2.0 ** -53 * abs(float(t_ref))
    assert abs(float(LD(t_got) - t_ref)) <= t_bar, (g, kind, float(t_got), float(t_ref), t_bar)


def test_order_is_the_documented_one():
    """Lane-strided ascending accumulation, then the tree: on values where the order of additions shows in the last bits, the replay
    differs from numpy's pairwise sum and from a plain left-to-right sum somewhere, and equals a scalar restatement everywhere."""
    differs = 0
    for g in SIZES:
        part = _parts(g, "squares")
        acc = [0.0] * 64
        for i, p in enumerate(part.tolist()):
            acc[i % 64] = acc[i % 64] + p
        v = list(acc)
        for step in (lambda i: i ^ 1, lambda i: i ^ 2, lambda i: (i & ~7) | (7 - (i & 7)), lambda i: (i & ~15) | (15 - (i & 15))):
            v = [v[i] + v[step(i)] for i in range(64)]
        scalar = (v[0] + v[16]) + (v[32] + v[48])
        assert S.start_sum(part) == scalar, g
        left = 0.0
        for p in part.tolist():
            left += p
        differs += int(S.start_sum(part) != left)
    assert differs > 0


@pytest.mark.parametrize("g", SIZES)
def test_a_dropped_partial_shows(g):
    """What the GPU test relies on: a sum that loses the last partial of any lane is not the replay's sum."""
    part = _parts(g, "squares") + 1.0
    full = S.start_sum(part)
    for lane in sorted({0, (g - 1) % 64, min(g, 64) - 1}):
        last = lane + 64 * ((g - 1 - lane) // 64)
        cut = part.copy()
        cut[last] = 0.0
        assert S.start_sum(cut) != full, (g, lane, last)
    assert S.tol2(part, 1.0, 0.0) == full and S.tol2(part, 0.0, 2.0) == 4.0
