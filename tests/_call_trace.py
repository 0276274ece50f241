"""The call trace of the batch Python API (osqp_amd/batch.py, osqp_amd/layer.py, the one-engine-per-member route): a
scripted session on faked handles whose library records every entry it is asked for -- name and arguments -- instead of
running it, and on the layers over recording stand-ins of BatchOSQP and OSQP.  Nothing here reaches a device.  The trace
says which C entry a public call reaches, with which scalars and with which array in which slot, what the call returns
(shapes and types) and what it raises (type and full text); tests/golden/batch_call_trace.json holds it as recorded on
the commit before osqp_amd/batch.py and layer.py got one body per call pair, and tests/test_batch_call_trace_host.py
replays the session and compares.

    python tests/_call_trace.py --write      # records the fixture from the tree this file lies in

Handles are faked as tests/test_batch_members_host.py fakes them; the shape is B = 4, n = 3, m = 2 (and m = 0),
nnzP = 4, nnzA = 5.  A session's steps are kept by label; sessions that give the same record for a label share it in the
fixture (merged() says how; sessions() has the short names of the sessions)."""
import ctypes as C
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _members_cases import DevArray      # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "batch_call_trace.json")
B, N, NNZP, NNZA = 4, 3, 4, 5
HANDLE = object()
# one fixed address per argument name, so that the trace shows which array went to which slot
NAMES = ("Q L U X Y info DX DY status_polish Px Ax dX dY dq dl du dPx dAx active status_adjoint dx dy dQ dL dU "
         "status_tangent").split()
ADDR = {name: 0x100 * (k + 1) for k, name in enumerate(NAMES)}
MEMBERS = dict(whole=None, two=[1, 3], mask=np.array([False, True, False, True]), all=list(range(B)))


# ---- recording -------------------------------------------------------------------------------------------------------
def _arg(a):
    if a is None:
        return "None"
    if a is HANDLE or isinstance(a, C.c_void_p):
        return "h"
    if isinstance(a, (bool, np.bool_)):
        return str(bool(a))
    if isinstance(a, (int, np.integer)):
        return "%d" % a if abs(int(a)) < 0x100 else hex(int(a))
    if isinstance(a, (float, np.floating)):
        return repr(float(a))
    if isinstance(a, C._Pointer):
        return "ptr" if bool(a) else "null"
    if type(a).__name__ == "CArgObject":          # ctypes.byref(...)
        return "ref"
    return type(a).__name__


class RecordingLib:
    """Stands for the library: every entry returns 0 -- or what `fail` holds for its name, or for "*" -- and appends
    "name(arguments)" to `calls`, the name without its osqp_amd_batch_ in front."""

    def __init__(self):
        self.calls, self.fail = [], {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append("%s(%s)" % (name.replace("osqp_amd_batch_", ""), ",".join(_arg(a) for a in args)))
            return self.fail.get(name, self.fail.get("*", 0))
        return call


def summary(v):
    """What a call returned: scalars as they are, arrays and tensors as type and shape, containers by member."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return v.item()
    short = lambda dtype, shape: "%s[%s]" % (dict(float64="f8", float32="f4", int64="i8", int32="i4").get(dtype, dtype),
                                             ",".join(str(d) for d in shape))
    if isinstance(v, np.ndarray):                # "f8[4,3]"; a tensor: "torch f8[4,3]"
        return short(str(v.dtype), v.shape)
    if type(v).__module__.startswith("torch"):
        return "torch " + short(str(v.dtype).replace("torch.", ""), v.shape) + ("" if v.is_contiguous() else " strided")
    if hasattr(v, "__cuda_array_interface__"):
        return "device%s" % list(v.__cuda_array_interface__["shape"])
    if hasattr(v, "_asdict"):
        return {k: summary(x) for k, x in v._asdict().items()}
    if isinstance(v, (tuple, list)):
        return [summary(x) for x in v]
    if isinstance(v, dict):
        return {str(k): summary(x) for k, x in v.items()}
    if hasattr(v, "__dict__"):
        return {k: summary(x) for k, x in sorted(vars(v).items()) if not k.startswith("_")}
    return type(v).__name__


class Session:
    def __init__(self, calls):
        self.calls, self.steps = calls, {}

    def step(self, label, fn):
        assert label not in self.steps, label
        del self.calls[:]
        try:
            out = summary(fn())
        except (ValueError, RuntimeError, TypeError) as e:
            out = "raises %s: %s" % (type(e).__name__, e)
        self.steps[label] = [list(self.calls), out]


def arrays(dev):
    """name, shape -> a zero host array, or a fake device array at the name's address."""
    def make(name, *shape, dtype=np.float64, fill=0.0):
        if dev:
            return DevArray(None, ADDR[name], tuple(shape), np.dtype(np.int32 if dtype is int else dtype))
        return np.full(shape, fill, dtype=np.int64 if dtype is int else dtype)
    return make


def subsets(names):
    """Nothing given, each one alone, all of them."""
    return [()] + [(k,) for k in names] + [tuple(names)]


def fake_handle(lib, engine, m, many=None, shared=True):
    from osqp_amd.batch import BatchOSQP
    h = BatchOSQP.__new__(BatchOSQP)
    h._lib, h._h, h._many, h._shared_kkt, h._status_polish = lib, HANDLE, many, shared, None
    h.engine, h.B, h.n, h.m = engine, B, N, m
    h.Pu, h.Ah = SimpleNamespace(nnz=NNZP), SimpleNamespace(nnz=NNZA if m else 0)
    return h


# ---- the scripted session of a kernel batch ----------------------------------------------------------------------------
def batch_session(engine, m, shared=True, many=None, member_forms=tuple(MEMBERS)):
    """A step's record is [the library calls it made, what it returned or raised]."""
    lib = RecordingLib()
    h = fake_handle(lib, engine, m, many, shared)
    s = Session(lib.calls)
    nA = h.Ah.nnz
    for dev, mname in itertools.product((False, True), member_forms):
        mem = MEMBERS[mname]
        a = arrays(dev)
        R = B if mem is None else int(np.count_nonzero(mem)) if mname == "mask" else len(mem)
        tag = "%s %s" % ("dev" if dev else "host", mname)
        kw = {} if mem is None else dict(members=mem)
        # every pattern of the optional arguments on the whole batch; with a list, nothing given and everything given
        some = (lambda patterns: patterns) if mem is None else (lambda patterns: [patterns[0], patterns[-1]])
        for given in some(subsets(("Q", "L", "U"))):
            s.step("update %s %s" % (tag, "+".join(given)), lambda: h.update(
                **{k: a(k, R, N if k == "Q" else m, fill=1.0 if k == "U" else 0.0) for k in given}, **kw))
        for given in some(subsets(("X", "Y"))):
            s.step("warm_start %s %s" % (tag, "+".join(given)), lambda: h.warm_start(
                **{k: a(k, R, N if k == "X" else m) for k in given}, **kw))
        # the derivative calls: [R, k] and [R, D = 2, k]
        for D in (None, 2):
            lead = (R,) if D is None else (R, D)
            form = "flat" if D is None else "D=2"
            cols = dict(dX=N, dY=m, dq=N, dl=m, du=m, dPx=NNZP, dAx=nA, dx=N, dy=m, dQ=N, dL=m, dU=m)
            f = lambda k: a(k, *lead, cols[k])
            if not dev:
                for with_dY, matrices in some(list(itertools.product((False, True), repeat=2))):
                    s.step("adjoint %s %s dY=%d matrices=%d" % (tag, form, with_dY, matrices), lambda: h.adjoint(
                        f("dX"), f("dY") if with_dY else None, matrices=matrices, **kw))
                for given in some(subsets(("dQ", "dL", "dU", "dPx", "dAx"))):
                    s.step("tangent %s %s %s" % (tag, form, "+".join(given)), lambda: h.tangent(**{k: f(k) for k in given}, **kw))
            else:
                for with_dY, extra in some(list(itertools.product((False, True), subsets(("dPx", "dAx", "active", "status_adjoint"))))):
                    opt = {k: f(k) for k in extra if k in cols}
                    if "active" in extra:
                        opt["active"] = a("active", R, m, dtype=int)
                    if "status_adjoint" in extra:
                        opt["status_adjoint"] = a("status_adjoint", R, dtype=int)
                    s.step("adjoint_into %s %s dY=%d %s" % (tag, form, with_dY, "+".join(extra)), lambda: h.adjoint_into(
                        f("dX"), f("dY") if with_dY else None, f("dq"), f("dl"), f("du"), **opt, **kw))
                s.step("adjoint_into %s %s no dl, du" % (tag, form), lambda: h.adjoint_into(f("dX"), None, f("dq"), None, None, **kw))
                s.step("adjoint_into %s %s no dX" % (tag, form), lambda: h.adjoint_into(None, None, f("dq"), f("dl"), f("du"), **kw))
                for given in some(subsets(("dQ", "dL", "dU", "dPx", "dAx", "active", "status_tangent"))):
                    opt = {k: f(k) for k in given if k in cols}
                    if "active" in given:
                        opt["active"] = a("active", R, m, dtype=int)
                    if "status_tangent" in given:
                        opt["status_tangent"] = a("status_tangent", R, dtype=int)
                    s.step("tangent_into %s %s %s" % (tag, form, "+".join(given)), lambda: h.tangent_into(f("dx"), f("dy"), **opt, **kw))
                s.step("tangent_into %s %s no dy" % (tag, form), lambda: h.tangent_into(f("dx"), None, dQ=f("dQ"), **kw))
                s.step("tangent_into %s %s no dx" % (tag, form), lambda: h.tangent_into(None, f("dy"), dQ=f("dQ"), **kw))
        if not dev:
            s.step("results %s" % tag, lambda: h.results(**kw))
            for fetch in (True, False):
                s.step("polish %s fetch=%d" % (tag, fetch), lambda: h.polish(fetch=fetch, **kw))
                s.step("results %s after polish fetch=%d" % (tag, fetch), lambda: h.results(**kw))
                for lim in some([{}, dict(max_iter=7), dict(time_limit=0.5), dict(max_iter=np.int64(9), time_limit=2)]):
                    s.step("solve %s fetch=%d %s" % (tag, fetch, "+".join(lim)), lambda: h.solve(fetch=fetch, **lim, **kw))
        else:
            for given in some(subsets(("X", "Y", "info", "DX", "DY", "status_polish"))):
                opt = {k: a(k, R, dict(X=N, Y=m, info=8, DX=N, DY=m).get(k)) for k in given if k != "status_polish"}
                if "status_polish" in given:
                    opt["status_polish"] = a("status_polish", B, dtype=int)
                s.step("results_into %s %s" % (tag, "+".join(given)), lambda: h.results_into(**opt, **kw))
    # new matrix values: shared and per member, with and without an index list, each of P and A given and not
    for dev in (False, True):
        a, tag = arrays(dev), "dev" if dev else "host"
        forms = dict(none=lambda nm, nnz: {}, shared=lambda nm, nnz: {nm: a(nm, nnz)}, per=lambda nm, nnz: {nm: a(nm, B, nnz)},
                     shared_idx=lambda nm, nnz: {nm: a(nm, 2), nm + "_idx": [0, nnz - 1]},
                     per_idx=lambda nm, nnz: {nm: a(nm, B, 2), nm + "_idx": np.array([1, 2])})
        for fp, fa in itertools.product(forms, repeat=2):
            if (nA < 3 and fa.endswith("idx")) or not (fa in ("none", "shared") or fp == "shared" or fp == fa):
                continue
            vals = dict(forms[fp]("Px", NNZP), **forms[fa]("Ax", nA))
            s.step("update_matrices %s P %s, A %s" % (tag, fp, fa), lambda: h.update_matrices(**vals))
            if not (fp.startswith("per") and fa.startswith("per")):
                s.step("update_model %s P %s, A %s" % (tag, fp, fa), lambda: h.update_model(**vals))
    s.step("update_rho scalar", lambda: h.update_rho(0.3))
    s.step("update_rho [B]", lambda: h.update_rho(np.full(B, 0.2)))
    for name in ("shape", "rounds", "solved_members", "solve_report", "columns", "kkt_info", "shared_kkt_peek", "device_arrays"):
        s.step(name, getattr(h, name))
    s.step("member_workspace", lambda: h.member_workspace(1))
    s.step("shared_kkt_peek qp=2", lambda: h.shared_kkt_peek(2))
    s.step("shared_kkt off", lambda: h.shared_kkt(False))
    s.step("polish after shared_kkt off", h.polish)
    s.step("shared_kkt on", lambda: h.shared_kkt(True))
    if m:                                   # (what is refused and how a code is worded does not look at m)
        refusals(s, h, m)
        return_codes(s, h, lib, m)
    h._shared_kkt = shared
    s.step("cleanup", h.cleanup)
    s.step("cleanup again", h.cleanup)
    return s.steps


def refusals(s, h, m):
    """What a form raises before any library call: mixed host and device arrays, each shape error, bad options."""
    host, dev = arrays(False), arrays(True)
    z = np.zeros
    nA = h.Ah.nnz
    cases = {
        "update mixed": lambda: h.update(Q=dev("Q", B, N), L=host("L", B, m)),
        "warm_start mixed": lambda: h.warm_start(X=host("X", B, N), Y=dev("Y", B, m)),
        "update_matrices mixed": lambda: h.update_matrices(Px=host("Px", NNZP), Ax=dev("Ax", B, nA)),
        "update_model mixed": lambda: h.update_model(Px=host("Px", NNZP), Ax=dev("Ax", nA)),
        "results_into host": lambda: h.results_into(X=host("X", B, N)),
        "results_into mixed": lambda: h.results_into(X=host("X", B, N), Y=dev("Y", B, m)),
        "adjoint_into host": lambda: h.adjoint_into(host("dX", B, N), None, host("dq", B, N), host("dl", B, m), host("du", B, m)),
        "adjoint_into mixed": lambda: h.adjoint_into(dev("dX", B, N), host("dY", B, m), dev("dq", B, N), dev("dl", B, m), dev("du", B, m)),
        "tangent_into host": lambda: h.tangent_into(host("dx", B, N), host("dy", B, m)),
        "tangent_into mixed": lambda: h.tangent_into(dev("dx", B, N), dev("dy", B, m), dQ=host("dQ", B, N)),
        "update shape Q": lambda: h.update(Q=z((B, N + 1))),
        "update shape L members": lambda: h.update(L=z((B, m)), members=[1, 3]),
        "update shape dev Q": lambda: h.update(Q=dev("Q", B, N + 1)),
        "update shape dev Q members": lambda: h.update(Q=dev("Q", B, N), members=[1, 3]),
        "update L > U": lambda: h.update(L=np.ones((B, m)), U=z((B, m))),
        "warm_start shape": lambda: h.warm_start(X=z(N)),
        "warm_start shape members": lambda: h.warm_start(Y=z((B, m)), members=[1, 3]),
        "warm_start shape dev members": lambda: h.warm_start(X=dev("X", B, N), members=[1, 3]),
        "update_matrices Px_idx alone": lambda: h.update_matrices(Px_idx=[0]),
        "update_matrices 3-D": lambda: h.update_matrices(Px=z((B, 1, NNZP))),
        "update_matrices rows": lambda: h.update_matrices(Px=z((B + 1, NNZP))),
        "update_matrices count": lambda: h.update_matrices(Px=z(NNZP - 1)),
        "update_matrices dev count": lambda: h.update_matrices(Px=dev("Px", B, NNZP + 1)),
        "update_matrices idx length": lambda: h.update_matrices(Px=z(2), Px_idx=[0]),
        "update_matrices idx range": lambda: h.update_matrices(Px=z(2), Px_idx=[0, NNZP]),
        "update_model per member": lambda: h.update_model(Px=z((B, NNZP))),
        "update_model dev per member": lambda: h.update_model(Px=dev("Px", B, NNZP)),
        "update_model count": lambda: h.update_model(Px=z(NNZP + 1)),
        "update_rho shape": lambda: h.update_rho(z(B + 1)),
        "solve max_iter 0": lambda: h.solve(max_iter=0),
        "solve max_iter bool": lambda: h.solve(max_iter=True),
        "solve time_limit inf": lambda: h.solve(time_limit=float("inf")),
        "solve time_limit 0": lambda: h.solve(time_limit=0),
        "solve members descending": lambda: h.solve(members=[3, 1]),
        "members empty": lambda: h.update(Q=z((0, N)), members=[]),
        "members range": lambda: h.results(members=[0, B]),
        "members mask length": lambda: h.polish(members=np.ones(B + 1, bool)),
        "members float": lambda: h.warm_start(X=z((2, N)), members=[0.5, 1.5]),
        "adjoint shape": lambda: h.adjoint(z((B, N + 1))),
        "adjoint shape dY": lambda: h.adjoint(z((B, N)), z((B, m + 1))),
        "adjoint shape members": lambda: h.adjoint(z((B, N)), members=[1, 3]),
        "adjoint multi shape": lambda: h.adjoint(z((B, 2, N + 1))),
        "adjoint multi shape members": lambda: h.adjoint(z((B, 2, N)), members=[1, 3]),
        "adjoint multi D differs": lambda: h.adjoint(z((B, 2, N)), z((B, 3, m))),
        "adjoint multi D = 0": lambda: h.adjoint(z((B, 0, N))),
        "adjoint_into dq shape": lambda: h.adjoint_into(dev("dX", B, N), None, dev("dq", B, N + 1), dev("dl", B, m), dev("du", B, m)),
        "adjoint_into dq shape members": lambda: h.adjoint_into(dev("dX", 2, N), None, dev("dq", B, N), dev("dl", 2, m),
                                                                dev("du", 2, m), members=[1, 3]),
        "adjoint_into multi shape members": lambda: h.adjoint_into(dev("dX", B, 2, N), None, dev("dq", B, 2, N), dev("dl", B, 2, m),
                                                                   dev("du", B, 2, m), members=[1, 3]),
        "adjoint_into multi D differs": lambda: h.adjoint_into(dev("dX", B, 2, N), None, dev("dq", B, 3, N), dev("dl", B, 2, m),
                                                               dev("du", B, 2, m)),
        "adjoint_into status type": lambda: h.adjoint_into(dev("dX", B, N), None, dev("dq", B, N), dev("dl", B, m), dev("du", B, m),
                                                           status_adjoint=dev("status_adjoint", B)),
        "tangent shape": lambda: h.tangent(dQ=z((B, N + 1))),
        "tangent shape members": lambda: h.tangent(dQ=z((B, N)), members=[1, 3]),
        "tangent forms differ": lambda: h.tangent(dQ=z((B, N)), dPx=z((B, 2, NNZP))),
        "tangent D differs": lambda: h.tangent(dQ=z((B, 3, N)), dPx=z((B, 2, NNZP))),
        "tangent_into dx shape": lambda: h.tangent_into(dev("dx", B, N + 1), dev("dy", B, m), dQ=dev("dQ", B, N)),
        "tangent_into shape members": lambda: h.tangent_into(dev("dx", B, N), dev("dy", B, m), dQ=dev("dQ", B, N), members=[1, 3]),
        "tangent_into forms differ": lambda: h.tangent_into(dev("dx", B, N), dev("dy", B, m), dQ=dev("dQ", B, 2, N)),
        "tangent_into status type": lambda: h.tangent_into(dev("dx", B, N), dev("dy", B, m), status_tangent=dev("status_tangent", B)),
        "results_into shape": lambda: h.results_into(X=dev("X", B, N + 1)),
        "results_into shape members": lambda: h.results_into(X=dev("X", B, N), members=[1, 3]),
        "results_into status_polish members": lambda: h.results_into(X=dev("X", 2, N), status_polish=dev("status_polish", B, dtype=int),
                                                                    members=[1, 3]),
        "results_into status_polish type": lambda: h.results_into(status_polish=dev("status_polish", B)),
    }
    for label, fn in cases.items():
        s.step("refusal: " + label, fn)


def return_codes(s, h, lib, m):
    """Each call's error path, once per code it words: the library returns 1, 5 or 7 from every entry, or from one."""
    host, dev = arrays(False), arrays(True)
    nA = h.Ah.nnz

    def into(kind, R, **kw):
        if kind == "adjoint":
            return h.adjoint_into(dev("dX", R, N), None, dev("dq", R, N), dev("dl", R, m), dev("du", R, m), **kw)
        return h.tangent_into(dev("dx", R, N), dev("dy", R, m), dQ=dev("dQ", R, N), **kw)
    calls = {
        "update": lambda: h.update(Q=host("Q", B, N)),
        "update dev members": lambda: h.update(Q=dev("Q", 2, N), members=[1, 3]),
        "warm_start": lambda: h.warm_start(X=host("X", B, N)),
        "update_matrices": lambda: h.update_matrices(Px=host("Px", NNZP)),
        "update_matrices dev": lambda: h.update_matrices(Px=dev("Px", NNZP)),
        "update_model": lambda: h.update_model(Px=host("Px", NNZP)),
        "update_model dev": lambda: h.update_model(Ax=dev("Ax", nA)),
        "update_rho": lambda: h.update_rho(1.0),
        "solve": h.solve,
        "solve limited": lambda: h.solve(max_iter=3),
        "solve members": lambda: h.solve(members=[1, 3]),
        "solve members limited": lambda: h.solve(members=[1, 3], time_limit=1.0),
        "polish": h.polish,
        "polish members": lambda: h.polish(members=[1, 3]),
        "adjoint": lambda: h.adjoint(host("dX", B, N)),
        "adjoint multi": lambda: h.adjoint(host("dX", B, 2, N)),
        "adjoint members": lambda: h.adjoint(host("dX", 2, N), members=[1, 3]),
        "adjoint_into": lambda: into("adjoint", B),
        "adjoint_into members": lambda: into("adjoint", 2, members=[1, 3]),
        "tangent": lambda: h.tangent(dQ=host("dQ", B, N)),
        "tangent members": lambda: h.tangent(dQ=host("dQ", 2, N), members=[1, 3]),
        "tangent_into": lambda: into("tangent", B),
        "tangent_into members": lambda: into("tangent", 2, members=[1, 3]),
        "results": h.results,
        "results members": lambda: h.results(members=[1, 3]),
        "results_into": lambda: h.results_into(X=dev("X", B, N)),
        "results_into members": lambda: h.results_into(X=dev("X", 2, N), members=[1, 3]),
        "shared_kkt": h.shared_kkt, "shared_kkt_peek": h.shared_kkt_peek, "shape": h.shape, "rounds": h.rounds,
        "solved_members": h.solved_members, "solve_report": h.solve_report, "columns": h.columns, "kkt_info": h.kkt_info,
        "member_workspace": lambda: h.member_workspace(1), "device_arrays": h.device_arrays,
    }
    shared = h._shared_kkt
    for code in (1, 5, 7):
        lib.fail = {"*": code}
        for label, fn in calls.items():
            # 5 stands for the codes a call only numbers; 1 and 7 go to the calls that word them
            if code == 5 or any(w in label for w in ("polish", "adjoint", "tangent", "into", "dev")):
                h._shared_kkt, h._status_polish = shared, None
                s.step("rc %d: %s" % (code, label), fn)
        lib.fail = {"osqp_amd_batch_polish_status_dev": code}
        h._shared_kkt, h._status_polish = shared, None
        s.step("rc %d: results_into status_polish" % code, lambda: h.results_into(status_polish=dev("status_polish", B, dtype=int)))

        def later():
            lib.fail = {}
            h.polish(fetch=False)
            lib.fail = {"osqp_amd_batch_polish": code}
            return h.results()
        s.step("rc %d: results after polish(fetch=False)" % code, later)
    lib.fail = {"osqp_amd_batch_common_update_model": 5, "osqp_amd_batch_common_kkt_peek": 4}
    h._shared_kkt = shared
    s.step("rc 5: update_model, the shared pieces went", lambda: (h.update_model(Px=host("Px", NNZP)), h._shared_kkt))
    lib.fail = {}
    h._shared_kkt, h._status_polish = shared, None


# ---- the one-engine-per-member route -------------------------------------------------------------------------------------
def many_refusals(m):
    """Every call a handle of the one-engine-per-member route refuses, on a handle faked as the host tests fake it
    (`_many = []`: the refusing paths look at nothing but `is not None`)."""
    lib = RecordingLib()
    h = fake_handle(lib, "auto", m, many=[])
    s = Session(lib.calls)
    host, dev = arrays(False), arrays(True)
    S = [1, 3]
    cases = {
        "update dev": lambda: h.update(Q=dev("Q", B, N)),
        "update members": lambda: h.update(Q=host("Q", 2, N), members=S),
        "warm_start dev": lambda: h.warm_start(X=dev("X", B, N)),
        "warm_start members": lambda: h.warm_start(X=host("X", 2, N), members=S),
        "update_matrices dev": lambda: h.update_matrices(Px=dev("Px", NNZP)),
        "update_model": lambda: h.update_model(Px=host("Px", NNZP)),
        "solve max_iter": lambda: h.solve(max_iter=5),
        "solve time_limit": lambda: h.solve(time_limit=1.0),
        "solve members": lambda: h.solve(members=S),
        "polish": h.polish,
        "polish members": lambda: h.polish(members=S),
        "adjoint": lambda: h.adjoint(host("dX", B, N)),
        "adjoint members": lambda: h.adjoint(host("dX", 2, N), members=S),
        "adjoint_into": lambda: h.adjoint_into(dev("dX", B, N), None, dev("dq", B, N), dev("dl", B, m), dev("du", B, m)),
        "tangent": lambda: h.tangent(dQ=host("dQ", B, N)),
        "tangent members": lambda: h.tangent(dQ=host("dQ", 2, N), members=S),
        "tangent_into": lambda: h.tangent_into(dev("dx", B, N), dev("dy", B, m)),
        "results members": lambda: h.results(members=S),
        "results_into": lambda: h.results_into(X=dev("X", B, N)),
        "solved_members": h.solved_members, "solve_report": h.solve_report, "kkt_info": h.kkt_info, "columns": h.columns,
        "shared_kkt": h.shared_kkt, "member_workspace": lambda: h.member_workspace(0), "device_arrays": h.device_arrays,
    }
    for label, fn in cases.items():
        s.step("refusal: " + label, fn)
    h._many = h._h = None
    return s.steps


class RecordingOSQP:
    """Stands for `OSQP` (osqp_amd/interface.py) under QPLayer and under the one-engine-per-member route: records method
    names, keyword names and the shapes and types of the arguments in `log` (shared by the objects of a session) and
    returns zeros of the right shapes.  `fail`: {(method, index of the object): what the method then returns or, for
    setup, raises}."""
    log, fail, count = [], {}, 0

    def __init__(self):
        cls = type(self)
        self.k = cls.count
        cls.count += 1

    def _rec(self, name, *args, **kw):
        type(self).log.append("OSQP[%d].%s(%s)" % (self.k, name, ", ".join(
            [json.dumps(summary(a)) for a in args] + ["%s=%s" % (k, json.dumps(summary(v))) for k, v in kw.items()])))
        return type(self).fail.get((name, self.k), 0)

    def setup(self, **kw):
        if self._rec("setup", **{k: (v.shape if hasattr(v, "tocsc") else v) for k, v in kw.items()}):
            raise ValueError("osqp_setup failed with error 5")
        self.n, self.m = kw["A"].shape[1], kw["A"].shape[0]
        self.nnz = (kw["P"].nnz, kw["A"].nnz)
        return self

    def update(self, **kw):
        return self._rec("update", **kw)

    def update_rho(self, rho):
        return self._rec("update_rho", rho)

    def warm_start(self, **kw):
        return self._rec("warm_start", **kw)

    def solve(self):
        self._rec("solve")
        z = np.zeros
        info = SimpleNamespace(iter=25, status_val=1, obj_val=0.0, pri_res=0.0, dua_res=0.0, rho_updates=0, rho_estimate=0.1)
        return SimpleNamespace(x=z(self.n), y=z(self.m), dual_inf_cert=z(self.n), prim_inf_cert=z(self.m), info=info)

    def settings(self):
        return SimpleNamespace(rho=0.1)

    def adjoint(self, dx, dy=None, matrices=False):
        self._rec("adjoint", dx, dy, matrices=matrices)
        z = np.zeros
        return SimpleNamespace(dq=z(self.n), dl=z(self.m), du=z(self.m), dPx=z(self.nnz[0]) if matrices else None,
                               dAx=z(self.nnz[1]) if matrices else None, status_adjoint=1, kkt_res=0.0)

    def tangent(self, *args):
        self._rec("tangent", *args)
        return SimpleNamespace(dx=np.zeros(self.n), dy=np.zeros(self.m), status_tangent=1, kkt_res=0.0)

    def cleanup(self):
        self._rec("cleanup")


def _fresh(cls, **fail):
    cls.log, cls.fail, cls.count = [], dict(fail), 0
    return cls.log


def many_session(m):
    """A handle of the one-engine-per-member route, set up through BatchOSQP.setup over recording stand-ins for OSQP (the
    size limit of the tiled kernel is lowered below n for the session), and the calls the route serves."""
    import osqp_amd
    import osqp_amd.batch as batch
    from scipy import sparse
    keep = osqp_amd.OSQP, batch.BATCH_MAX_N, osqp_amd.engine_options, osqp_amd.set_engine_options
    options = dict(device=0)
    log = _fresh(RecordingOSQP)
    osqp_amd.OSQP, batch.BATCH_MAX_N = RecordingOSQP, 2
    osqp_amd.engine_options = lambda: dict(options)
    osqp_amd.set_engine_options = lambda **kw: (log.append("set_engine_options(%s)" % json.dumps(kw)), options.update(kw))[0]
    try:
        lib = RecordingLib()
        s = Session(log)
        P = sparse.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))      # triu: nnzP = 4
        A = sparse.csc_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]])[:m] if m else np.zeros((0, N)))
        nA = A.nnz
        z = np.zeros

        def new():
            h = batch.BatchOSQP.__new__(batch.BatchOSQP)
            h._lib, h._h, h._status_polish = lib, None, None
            return h

        def setup(h, **kw):
            return h.setup(P, A, z((B, N)), z((B, m)), np.ones((B, m)), **kw) is h
        h = new()
        s.step("setup", lambda: setup(h, device=1, eps_abs=1e-5))
        s.step("setup left", lambda: dict(B=h.B, n=h.n, m=h.m, many=h._many is not None, h=h._h is None, engine=h.engine,
                                          device=options["device"]))
        h2 = new()
        s.step("setup with values", lambda: setup(h2, Px_all=np.ones((B, NNZP)), Ax_all=np.ones((B, nA))))
        RecordingOSQP.fail[("setup", RecordingOSQP.count + 2)] = 1
        h3 = new()
        s.step("setup, member 2 fails", lambda: setup(h3))
        s.step("setup, member 2 fails: left", lambda: dict(many=h3._many is not None, device=options["device"]))
        RecordingOSQP.fail.clear()
        for given in subsets(("Q", "L", "U")):
            s.step("update " + "+".join(given), lambda: h.update(**{k: np.full((B, N if k == "Q" else m), float(k == "U"))
                                                                    for k in given}))
        s.step("update L > U", lambda: h.update(L=np.ones((B, m)), U=z((B, m))))
        s.step("update shape", lambda: h.update(Q=z((B, N + 1))))
        for fp, fa in itertools.product(("none", "shared", "per", "shared_idx", "per_idx"), repeat=2):
            if nA < 3 and fa.endswith("idx"):
                continue
            vals = {}
            for nm, form, nnz in (("Px", fp, NNZP), ("Ax", fa, nA)):
                if form != "none":
                    vals[nm] = z((B, 2) if form == "per_idx" else (2,) if form == "shared_idx" else (B, nnz) if form == "per" else (nnz,))
                if form.endswith("idx"):
                    vals[nm + "_idx"] = [0, nnz - 1]
            s.step("update_matrices P %s, A %s" % (fp, fa), lambda: h.update_matrices(**vals))
        s.step("update_matrices count", lambda: h.update_matrices(Px=z(NNZP + 1)))
        s.step("update_rho scalar", lambda: h.update_rho(0.3))
        s.step("update_rho [B]", lambda: h.update_rho(np.arange(1.0, B + 1)))
        s.step("update_rho <= 0", lambda: h.update_rho(np.array([1.0, 0.0, 1.0, 1.0])))
        s.step("update_rho shape", lambda: h.update_rho(z(B + 1)))
        for given in subsets(("X", "Y")):
            s.step("warm_start " + "+".join(given), lambda: h.warm_start(**{k: z((B, N if k == "X" else m)) for k in given}))
        s.step("warm_start shape", lambda: h.warm_start(X=z((B + 1, N))))
        # a member that returns a non-zero code: the code comes back and last_update_failed says who it was
        for label, call, fn in (("update", "update", lambda: h.update(Q=z((B, N)))),
                                ("update_matrices", "update", lambda: h.update_matrices(Px=z(NNZP))),
                                ("update_rho", "update_rho", lambda: h.update_rho(0.5)),
                                ("warm_start", "warm_start", lambda: h.warm_start(X=z((B, N))))):
            RecordingOSQP.fail = {(call, 2): 3}
            s.step("%s, member 2 returns 3" % label, lambda: (fn(), h.last_update_failed))
        RecordingOSQP.fail = {}
        s.step("update after a failure", lambda: (h.update(Q=z((B, N))), h.last_update_failed))
        s.step("solve fetch=False", lambda: h.solve(fetch=False))
        s.step("results", h.results)
        s.step("solve", h.solve)
        s.step("cleanup", h.cleanup)
        s.step("cleanup left", lambda: dict(many=h._many is not None))
        s.step("cleanup again", h.cleanup)
        h2.cleanup()
        return s.steps
    finally:
        osqp_amd.OSQP, batch.BATCH_MAX_N, osqp_amd.engine_options, osqp_amd.set_engine_options = keep


def setup_session(m):
    """BatchOSQP.setup of the three engines over the recording library."""
    import osqp_amd.batch as batch
    from scipy import sparse
    lib = RecordingLib()
    s = Session(lib.calls)
    P = sparse.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))
    A = sparse.csc_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]])[:m] if m else np.zeros((0, N)))
    z = np.zeros
    made = []

    def setup(**kw):
        h = batch.BatchOSQP.__new__(batch.BatchOSQP)
        h._lib, h._h, h._status_polish = lib, None, None
        made.append(h)
        h.setup(P, A, z((B, N)), z((B, m)), np.ones((B, m)), device=0, **kw)
        return dict(engine=h.engine, many=h._many is not None, shared=h._shared_kkt, B=h.B, n=h.n, m=h.m)
    cases = {
        "auto": dict(), "auto with values": dict(Px_all=np.ones((B, NNZP)), Ax_all=np.ones((B, A.nnz))),
        "streamed": dict(engine="streamed", eps_abs=1e-5), "common": dict(engine="common"),
        "common shared": dict(engine="common", shared_kkt=True),
        "bad engine": dict(engine="tiled"), "common with values": dict(engine="common", Px_all=np.ones((B, NNZP))),
        "shared_kkt on streamed": dict(engine="streamed", shared_kkt=True), "polish setting": dict(polish=1),
        "time_limit setting": dict(time_limit=1.0), "unknown setting": dict(epsilon=1.0), "Px_all shape": dict(Px_all=z((B, NNZP + 1))),
    }
    for label, kw in cases.items():
        s.step("setup " + label, lambda: setup(**kw))
    for code in (1, 5):
        lib.fail = {"*": code}
        for engine in ("auto", "streamed", "common"):
            s.step("rc %d: setup %s" % (code, engine), lambda: setup(engine=engine))
    lib.fail = {"osqp_amd_batch_common_kkt": 5}
    s.step("rc 5: setup common, shared pieces", lambda: setup(engine="common", shared_kkt=True))
    lib.fail = {}
    s.step("BatchOSQP()", lambda: type(batch.BatchOSQP()._lib).__name__)
    for h in made:
        h._h = None
        if not hasattr(h, "_many"):
            h._many = None
    return s.steps


# ---- the layers --------------------------------------------------------------------------------------------------------
class RecordingBatch:
    """Stands for BatchOSQP under BatchQPLayer: records method names, keyword names, and the shapes and types of the
    arguments, and returns zeros of the right shapes."""
    log = []

    def _rec(self, name, *args, **kw):
        type(self).log.append("BatchOSQP.%s(%s)" % (name, ", ".join(
            [json.dumps(summary(a)) for a in args] + ["%s=%s" % (k, json.dumps(summary(v))) for k, v in kw.items()])))

    def setup(self, P, A, Q, L, U, **kw):
        self._rec("setup", P.shape, A.shape, Q, L, U, **kw)
        self.B, self.n, self.m = Q.shape[0], Q.shape[1], A.shape[0]
        self.Pu, self.Ah = SimpleNamespace(nnz=NNZP), SimpleNamespace(nnz=A.nnz)
        return self

    def update(self, **kw):
        self._rec("update", **kw)
        return 0

    def update_matrices(self, **kw):
        self._rec("update_matrices", **kw)
        return 0

    def update_model(self, **kw):
        self._rec("update_model", **kw)
        return 0

    def solve(self, **kw):
        self._rec("solve", **kw)

    def results(self):
        self._rec("results")
        z = np.zeros
        return SimpleNamespace(x=z((self.B, self.n)), y=z((self.B, self.m)), status_polish=z(self.B, np.int64))

    def polish(self, **kw):
        self._rec("polish", **kw)
        return SimpleNamespace(x=np.zeros((self.B, self.n)), y=np.zeros((self.B, self.m)), status_polish=np.ones(self.B, np.int64))

    def adjoint(self, dX, dY=None, matrices=False):
        self._rec("adjoint", dX, dY, matrices=matrices)
        z = lambda k: np.zeros((self.B, k))
        return SimpleNamespace(dq=z(self.n), dl=z(self.m), du=z(self.m), dPx=z(self.Pu.nnz) if matrices else None,
                               dAx=z(self.Ah.nnz) if matrices else None, status_adjoint=np.ones(self.B, np.int64))

    def tangent(self, *args):
        self._rec("tangent", *args)
        return SimpleNamespace(dx=np.zeros((self.B, self.n)), dy=np.zeros((self.B, self.m)), status_tangent=np.ones(self.B, np.int64))

    def cleanup(self):
        self._rec("cleanup")


def layer_session(kind, m):
    """kind: "auto" / "common" (BatchQPLayer of that engine) or "single" (QPLayer), on CPU tensors over the recording
    stand-ins: forward and backward with every requires_grad pattern of the five inputs, forward mode, a second forward
    that no longer gives Px / Ax, then the backward of the first graph (the handle has to bring its problem back), and
    the refusals of forward."""
    import torch
    import torch.autograd.forward_ad as fwAD
    import osqp_amd
    import osqp_amd.layer as layer
    from scipy import sparse
    keep = osqp_amd.OSQP, layer.BatchOSQP, getattr(layer, "_hand_over", None)
    log = RecordingBatch.log = _fresh(RecordingOSQP)
    osqp_amd.OSQP, layer.BatchOSQP = RecordingOSQP, RecordingBatch
    layer._hand_over = lambda device: log.append("hand-over")
    try:
        s = Session(log)
        P = sparse.csc_matrix(np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))
        A = sparse.csc_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]])[:m] if m else np.zeros((0, N)))
        nA = A.nnz
        single, common = kind == "single", kind == "common"
        lead = () if single else (B,)
        vlead = () if single or common else (B,)
        shapes = dict(Q=lead + (N,), L=lead + (m,), U=lead + (m,), Px=vlead + (NNZP,), Ax=vlead + (nA,))

        def make():
            if single:
                return layer.QPLayer(P, A, eps_abs=1e-6)
            return layer.BatchQPLayer(P, A, engine=kind, **(dict(shared_kkt=True) if common else {}))

        def inputs(grad, given=("Px", "Ax")):
            t = {k: torch.full(shapes[k], 1.0 if k == "U" else 0.0, dtype=torch.float64, requires_grad=k in grad) for k in shapes}
            return t["Q"], t["L"], t["U"], (t["Px"] if "Px" in given else None), (t["Ax"] if "Ax" in given else None)

        def status(lay):
            return {k: summary(getattr(lay, k, "absent")) for k in ("last_results", "last_status_adjoint", "last_status_tangent",
                                                                    "last_kkt_res", "last_route", "_own", "_serial")}
        lay = make()
        for r in range(6) if m else (0, 1, 5):
            for grad in itertools.combinations(shapes, r):
                def run():
                    args = inputs(grad)
                    X, Y = lay(*args, return_y=True)
                    if grad:
                        (X.sum() + Y.sum()).backward()
                    if r in (0, 5):
                        return dict(X=X, Y=Y, grads=[a.grad for a in args], status=status(lay))
                    before = len(log) - 1     # (the calls of forward are those of the two patterns above: their number and adjoint stay)
                    del log[:-1]
                    return dict(calls_before=before, grads=[a.grad for a in args])
                s.step("forward, backward: grad %s" % "+".join(grad), run)

        def one_output(which):
            args = inputs(("Q", "Ax"))
            X, Y = lay(*args, return_y=True)
            (X if which == "X" else Y).sum().backward()
            return [a.grad for a in args]
        s.step("backward of X alone", lambda: one_output("X"))
        s.step("backward of Y alone", lambda: one_output("Y"))
        s.step("forward without return_y", lambda: lay(*inputs(())[:3]))
        for with_t in (("Q", "L", "U", "Px", "Ax"), ("Q",), ("Ax",)):
            def forward_mode():
                with fwAD.dual_level():
                    args = [fwAD.make_dual(a, torch.ones_like(a)) if k in with_t else a for k, a in zip(shapes, inputs(()))]
                    X, Y = lay(*args, return_y=True)
                    return dict(X=X, tX=fwAD.unpack_dual(X).tangent, tY=fwAD.unpack_dual(Y).tangent, status=status(lay))
            s.step("forward mode: tangents of %s" % "+".join(with_t), forward_mode)
        graphs = {}

        def first():
            graphs["args"] = inputs(("Q", "L", "Px"))
            graphs["X"] = lay(*graphs["args"])
            return status(lay)
        s.step("first graph: Px, Ax given", first)
        s.step("second forward: Px given, Ax not", lambda: (lay(*inputs((), given=("Px",))), status(lay))[1])
        s.step("third forward: neither given", lambda: (lay(*inputs((), given=())), status(lay))[1])
        s.step("fourth forward: neither given", lambda: (lay(*inputs((), given=())), status(lay))[1])

        def back():
            graphs["X"].sum().backward()
            return dict(grads=[a.grad for a in graphs["args"]], status=status(lay))
        s.step("backward of the first graph: bring it back", back)
        if not single:
            s.step("forward with another B", lambda: lay(*(torch.zeros((B + 1,) + shapes[k][1:], dtype=torch.float64) for k in "QLU")))
        f32 = lambda k: torch.zeros(shapes[k], dtype=torch.float32)
        f64 = lambda k, *shape: torch.zeros(shape or shapes[k], dtype=torch.float64)
        refusals = {
            "dtype": lambda: lay(f32("Q"), f64("L"), f64("U")),
            "shape of L": lambda: lay(f64("Q"), f64("L", *(lead + (m + 1,))), f64("U")),
            "shape of Px": lambda: lay(f64("Q"), f64("L"), f64("U"), Px=f64("Px", *(vlead + (NNZP + 1,)))),
            "Px with another leading shape": lambda: lay(f64("Q"), f64("L"), f64("U"), Px=f64("Px", *((() if vlead else (B,)) + (NNZP,)))),
            "Q of one dimension more": lambda: lay(f64("Q", *((2,) + shapes["Q"])), f64("L"), f64("U")),
        }
        for label, fn in refusals.items():
            s.step("refusal: " + label, fn)
        s.step("cleanup", lay.cleanup)
        s.step("cleanup again", lay.cleanup)
        if not single:
            s.step("common without shared_kkt", lambda: layer.BatchQPLayer(P, A, engine="common") and None)
        return s.steps
    finally:
        osqp_amd.OSQP, layer.BatchOSQP = keep[:2]
        if keep[2] is None:
            del layer._hand_over
        else:
            layer._hand_over = keep[2]


# ---- the whole trace ---------------------------------------------------------------------------------------------------
def sessions():
    """By short name: t / s / k / c = tiled, streamed, common-K with and without its shared pieces; r / p = the refusals
    and the calls of the one-engine-per-member route; u = setup; la / lc / ls = BatchQPLayer "auto" and "common", QPLayer;
    the digit is m."""
    out = {}
    for m in (2, 0):
        forms = tuple(MEMBERS) if m else ("whole", "two")
        out["t%d" % m] = batch_session("auto", m, member_forms=forms)
        out["s%d" % m] = batch_session("streamed", m, member_forms=forms)
        out["k%d" % m] = batch_session("common", m, shared=True, member_forms=forms)
        out["c%d" % m] = batch_session("common", m, shared=False, member_forms=("whole", "two"))      # (all refusals)
        out["p%d" % m] = many_session(m)
        out["u%d" % m] = setup_session(m)
    out["r2"] = many_refusals(2)
    out.update(la2=layer_session("auto", 2), lc2=layer_session("common", 2), ls2=layer_session("single", 2),
               la0=layer_session("auto", 0))
    return out


def merged(all_sessions):
    """{"records": the distinct records, "steps": {label: [[index of the record, "the sessions that gave it"], ...], or the
    [index, number of sessions] where every session that has the step gave one record}}: most records are the same on every engine, and
    many steps are refused in the same words."""
    records, steps = [], {}
    for name, session in all_sessions.items():
        for label, record in session.items():
            record = json.loads(json.dumps(record))      # (as the fixture reads back: tuples are lists)
            if record not in records:
                records.append(record)
            k = records.index(record)
            for entry in steps.setdefault(label, []):
                if entry[0] == k:
                    entry[1] += " " + name
                    break
            else:
                steps[label].append([k, name])
    return dict(records=records, steps={label: [e[0][0], e[0][1].count(" ") + 1] if len(e) == 1 else e for label, e in steps.items()})


def trace():
    """{label: [[record, "sessions"], ...]} of the sessions run now."""
    return expand(merged(sessions()))


def expand(fixture):
    return {label: [[fixture["records"][e[0]], e[1]] for e in ([entries] if isinstance(entries[0], int) else entries)]
            for label, entries in fixture["steps"].items()}


def write(path=FIXTURE):
    t = merged(sessions())
    with open(path, "w") as f:
        f.write('{"records": [\n' + ",\n".join(json.dumps(r) for r in t["records"]) + '\n],\n"steps": {')
        width = 0
        for k, (label, entries) in enumerate(t["steps"].items()):       # (several steps on a line of the usual width)
            item = "%s: %s%s" % (json.dumps(label), json.dumps(entries), "," if k + 1 < len(t["steps"]) else "")
            width = width + len(item) + 1 if width and width + len(item) < 130 else 0
            f.write((" " if width else "\n") + item)
            width = width or len(item)
        f.write("\n}}\n")
    return t


if __name__ == "__main__":
    if "--write" in sys.argv[1:]:
        t = write()
        print("%s: %d labels, %d records, %d bytes" % (FIXTURE, len(t["steps"]), len(t["records"]), os.path.getsize(FIXTURE)))
    else:
        print(json.dumps(trace(), indent=1))
