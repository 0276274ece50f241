"""Cases of the common-K engine's packed and chosen-member solves (tests/test_gpu_batch_common_members.py), proved on
the CPU by tests/test_common_members_cases_host.py.

Wave case W: `common_family(17, 37, B, 1054)` under FIXED with a chosen set of members made trivially easy -- q = 0 and
every bound shifted by -A x0_b, so that it contains 0 (an equality row becomes l = u = 0, an infinite bound stays
infinite).  From a cold start such a member sits at the optimum x = 0 and ends at the first check point, iteration 25;
the other ("hard") members end in waves at later check points.  The easy members have q = 0, so q^ of the batch is
q^ of the hard members alone: a handle set up on the hard members has the batch's scaling to the bit.

A wave case is named by (B, h, drop): the hard members are the first h even-indexed ones, 0, 2, ..., 2 (h - 1), without
those listed in `drop`; every odd member, every member from 2 h on and the dropped ones are easy -- the easy members
interleave with the hard ones and end in a block.  `drop` takes out a member that would come closer to a termination
threshold than MARGIN_CHECK, or trims the number running after iteration 25 to the one a test is about.

Adaptive subset case: `adaptive_family(33, 66, B, 100.0)` under ADAPTIVE with Q of the members outside the chosen set
S clipped element-wise to +-q^(Q[S]), so that q^(Q) == q^(Q[S]): a handle set up on S alone has the batch's scaling."""
import numpy as np

from _common_cases import FIXED, adaptive_family, common_family, qhat

WAVE_N, WAVE_M, WAVE_SEED = 17, 37, 1054
GROUP = 64                 # BC_TX = BC_TILE: the columns of a workgroup of every kernel of the solve
PACK_CHUNK = 256           # k_bc_pack walks a row in chunks of this many columns
MIN_ITER = 25              # the first check point: where an easy member ends
# name: (B, h, drop) of the GPU tests, with what the host test proves of each -- the members still running after
# iteration 25 (the columns the first pack leaves) and the number of packs.  "one": one pack, 130 -> 45 columns.
# "two": 200 -> 93 -> 14.  "chunk": 600 -> 290 columns, more than a chunk of k_bc_pack, then two packs more (member 412
# comes within 7e-4 of a threshold at iteration 50 and is made easy).  "to-64", "to-65", "to-17": the first pack leaves
# exactly that many columns.
WAVES = {
    "one": (130, 50, ()),
    "two": (200, 100, ()),
    "chunk": (600, 300, (412,)),
    "to-64": (150, 69, (2,)),
    "to-65": (150, 69, ()),
    "to-17": (150, 18, ()),
}
WAVE_PROVED = {"one": (45, 1), "two": (93, 2), "chunk": (290, 3), "to-64": (64, 1), "to-65": (65, 2), "to-17": (17, 1)}


def wave_hard(B, h, drop=()):
    hard = np.setdiff1d(2 * np.arange(h), drop)
    assert hard[-1] < B
    return hard


def wave_case(B, h, drop=()):
    """(P, A, Q, L, U, hard): the wave case (B, h, drop) and the indices of its hard members."""
    P, A, Q, L, U, X0 = common_family(WAVE_N, WAVE_M, B, WAVE_SEED)
    hard = wave_hard(B, h, drop)
    easy = np.setdiff1d(np.arange(B), hard)
    for b in easy:
        ax = A @ X0[b]
        Q[b] = 0.0
        L[b] = L[b] - ax          # (-inf stays -inf; an equality row, L = U = ax, becomes exactly 0)
        U[b] = U[b] - ax
    return P, A, Q, L, U, hard


def packs_of(iters, B=None):
    """(packs, columns in use at the end) the engine's rule makes of members that end at the iterations `iters` (check
    points, in member order): after a check point with Rn members still running of C columns in use, it packs when
    ceil(Rn / 64) < ceil(C / 64) and Rn > 0."""
    iters = np.asarray(iters)
    C = iters.size if B is None else B
    packs = 0
    for it in sorted(set(iters.tolist())):
        Rn = int((iters > it).sum())
        if Rn > 0 and -(-Rn // GROUP) < -(-C // GROUP):
            packs += 1
            C = Rn
    return packs, C


_WAVE_RUNS = {}


def wave_reference(orc, B, h, drop=()):
    """The long-double reference run of the wave case (B, h, drop): (reference after its run, result); computed once per
    process and shared -- callers leave both unchanged."""
    from _common_reference import reference_for
    if (B, h, drop) not in _WAVE_RUNS:
        P, A, Q, L, U, _ = wave_case(B, h, drop)
        ref = reference_for(orc, P, A, Q, L, U, **FIXED)
        _WAVE_RUNS[B, h, drop] = (ref, ref.solve())
    return _WAVE_RUNS[B, h, drop]


ADAPTIVE_SUBSET_B = 130


def adaptive_subset_case(S, B=ADAPTIVE_SUBSET_B):
    """(P, A, Q, L, U) of the adaptive subset case for the chosen members S."""
    P, A, Q, L, U, _ = adaptive_family(33, 66, B, 100.0)
    S = np.asarray(S)
    cap = qhat(Q[S])
    rest = np.setdiff1d(np.arange(B), S)
    Q[rest] = np.clip(Q[rest], -cap, cap)
    return P, A, Q, L, U


def subsets(B):
    """The chosen-member sets of the subset tests: |S| = 1, 16, 17, 63, 64, 65 at the front, at the back and strided."""
    out = []
    for k in (1, 16, 17, 63, 64, 65):
        out.append(("front-%d" % k, np.arange(k)))
        out.append(("back-%d" % k, np.arange(B - k, B)))
        out.append(("strided-%d" % k, np.arange(k) * 2))
    return out
