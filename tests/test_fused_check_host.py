"""hipeng_early_scalars_usable (engine.hip) without a device: the rule by which hipeng_run_admm_check keeps the residual scalars it
took directly behind a window's graphs.  They belong to the iterate the call ends on only if the window did all it was asked for
(remaining == 0: no stall continuation was left), no resident launch gave up (State::res_fail) and no slow-wait record had to be
cleared (State::res_slow, State::res_repub).  Every branch, and every combination of the four inputs."""
import ctypes as C
import itertools


def _rule():
    import osqp_amd
    f = osqp_amd.lib().hipeng_early_scalars_usable
    f.restype, f.argtypes = C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int]
    return f


def test_each_branch():
    f = _rule()
    assert f(0, 0, 0, 0) == 1
    assert f(1, 0, 0, 0) == 0           # a continuation is left to run
    assert f(0, 1, 0, 0) == 0           # a resident launch gave up
    assert f(0, 0, 1, 0) == 0           # slow waits on record
    assert f(0, 0, 0, 1) == 0           # re-publications on record


def test_every_combination():
    f = _rule()
    for rem, fail, slow, repub in itertools.product((0, 1, 24, 128), (0, 1), (0, 1, 7), (0, 1, 3)):
        assert f(rem, fail, slow, repub) == int(rem == 0 and not fail and not slow and not repub), (rem, fail, slow, repub)
