"""The single-QP engine's table of OSQP_AMD_* switches (csrc/engine.hip, ahead of struct hipeng) from outside, without a device:
its rows, what its reader makes of the environment (defaults, clamps, ignored values, "unset" as a value of its own), and that
nothing else names a switch the table does not have -- the Python restatement of the selection cascade, the tests and tools that
set switches, and the environment section of INTEGRATION.md are all held to it."""
import ctypes as C
import glob
import os
import re

import pytest

import osqp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG, INT, DOUBLE, PAIR, TEXT = range(5)
UNSET = -1.0
PROBLEM_DEPENDENT = ("SPLIT", "DENSE_SYMV", "FIN_GRID", "CHUNK")      # unset: worked out from the problem
# not switches of the library: read by osqp_amd/batch.py; the peek selectors of the row-partitioned tests (a prefix); build macros
ALLOWED = {"OSQP_AMD_BATCH_TILED", "OSQP_AMD_TIMELINE", "OSQP_AMD_BATCH_DEBUG"}
ALLOWED_PREFIX = "OSQP_AMD_RP_PEEK_"


def _lib():
    L = osqp_amd.lib()
    L.hipeng_switch_row.restype = C.c_int
    L.hipeng_switch_row.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_char_p)]
    L.hipeng_switch_values.restype = C.c_int
    L.hipeng_switch_values.argtypes = [C.POINTER(C.c_double), C.c_int]
    return L


def table():
    """[(name, kind, default text, unset is distinct, description)] in the table's order"""
    L = _lib()
    rows = []
    for i in range(L.hipeng_switch_row(-1, None, None, None, 0, None, None)):
        name, what, kind, unset, text = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.create_string_buffer(64)
        L.hipeng_switch_row(i, C.byref(name), C.byref(kind), text, 64, C.byref(unset), C.byref(what))
        rows.append((name.value.decode(), kind.value, text.value.decode(), bool(unset.value), what.value.decode()))
    return rows


def values():
    """{short name: value} under the current environment; a pair reads as a tuple"""
    L = _lib()
    rows = table()
    out = (C.c_double * (2 * len(rows)))()
    assert L.hipeng_switch_values(out, len(rows)) == len(rows)
    return {r[0][len("OSQP_AMD_"):]: ((out[2 * i], out[2 * i + 1]) if r[1] == PAIR else out[2 * i]) for i, r in enumerate(rows)}


def _source_names(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return set(re.findall(r'getenv\("(OSQP_AMD_[A-Z0-9_]+)"\)', f.read()))


def other_library_names():
    """the switches of the batch engines (fill_settings) and of the C host side (opt_init), from their sources"""
    names = _source_names("osqp_amd/csrc/batch.hip") | _source_names("osqp_amd/csrc/osqp_host.c")
    assert len(names) >= 10, names
    return names


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("OSQP_AMD_"):
            monkeypatch.delenv(k)
    return monkeypatch


def test_table_rows():
    rows = table()
    names = [r[0] for r in rows]
    assert len(rows) == 39
    assert len(set(names)) == 39 and all(n.startswith("OSQP_AMD_") and len(n) > len("OSQP_AMD_") for n in names)
    assert not set(names) & other_library_names()
    assert all(r[1] in (FLAG, INT, DOUBLE, PAIR, TEXT) and r[4] for r in rows)
    distinct = {r[0][len("OSQP_AMD_"):] for r in rows if r[3]}
    assert set(PROBLEM_DEPENDENT) <= distinct and distinct == set(PROBLEM_DEPENDENT) | {"SETUP_THREADS", "DENSE_CHOL"}
    assert all(r[2] == "unset" for r in rows if r[3])


def test_values_with_nothing_set(clean_env):
    v = values()
    assert v == dict(
        RESIDENT=1, RESIDENT_MIN_N=256, RESIDENT_ALL_CUS=0, RESIDENT_NWG=0, RESIDENT_BANKS=1, RESIDENT_PIPE=1, RESIDENT_PREDICT=1,
        RESIDENT_PREDICT_MARGIN=1.0, RESIDENT_INJECT=0, RESIDENT_U0=1, RESIDENT_FINE=2, RESIDENT_BLOCKS=1, INIT_RESIDENT_STORES=1,
        FORM_K_LISTS=1, FORM_K_LIST_MB=128.0, SETUP_THREADS=UNSET, BLOCK_DIRECT=1, BLOCK_COUPLED_MAX=512, BLOCK_FIN_DOTS=1, BLOCK_PLAIN=0,
        DENSE_P=1, DENSE_DIRECT=1, DENSE_SMALL=1024, DENSE_SYMV=UNSET, DENSE_ONE_GATHER=1, DENSE_CHOL=UNSET, DENSE_GEMM_LDS=1, ELIM=1,
        HFOLD=1, SPLIT=UNSET, CHUNK=UNSET, FIN_GRID=UNSET, FUSED_CHECK=1, EXTRAP=1.0, EXTRAP_SCHED=(5.0, 12.0), KHEAD=1, GRAPH_SEGS=5,
        TRACE=0, TRACE_MAPS=0)
    # the default column of the table says the same (a row where unset is distinct says "unset")
    for name, kind, text, unset, _ in table():
        got = v[name[len("OSQP_AMD_"):]]
        if unset:
            assert got == UNSET
        elif kind == PAIR:
            assert tuple(float(t) for t in text.split(",")) == got
        elif kind == TEXT:
            assert text == "" and got == 0
        else:
            assert float(text) == got


@pytest.mark.parametrize("name,text,want", [
    ("CHUNK", "32", UNSET), ("CHUNK", "4096", UNSET), ("CHUNK", "64", 64), ("CHUNK", "2048", 2048),
    ("SETUP_THREADS", "0", 1), ("SETUP_THREADS", "999", 64), ("SETUP_THREADS", "3", 3),
    ("FORM_K_LIST_MB", "-1", 0.0), ("FORM_K_LIST_MB", "2e6", 1e6), ("FORM_K_LIST_MB", "0.5", 0.5),
    ("GRAPH_SEGS", "0", 1), ("GRAPH_SEGS", "99", 32), ("GRAPH_SEGS", "1", 1),
    ("BLOCK_COUPLED_MAX", "9999", 512), ("BLOCK_COUPLED_MAX", "-3", 0), ("BLOCK_COUPLED_MAX", "17", 17),
    ("RESIDENT_PREDICT_MARGIN", "0", 1.0), ("RESIDENT_PREDICT_MARGIN", "-1", 1.0), ("RESIDENT_PREDICT_MARGIN", "1e30", 1e30),
    ("TRACE", "0", 1), ("TRACE", "2", 2), ("TRACE", "", 1),
    ("EXTRAP_SCHED", "1,2", (1.0, 2.0)), ("EXTRAP_SCHED", "7", (7.0, 12.0)), ("EXTRAP_SCHED", "x", (5.0, 12.0)),
    ("RESIDENT_MIN_N", "abc", 0), ("KHEAD", "abc", 0), ("DENSE_DIRECT", "abc", 0), ("RESIDENT", "abc", 0), ("EXTRAP", "abc", 0.0),
    ("DENSE_DIRECT", "2", 2), ("DENSE_SMALL", "-5", 0), ("FIN_GRID", "0", 1), ("FIN_GRID", "300", 300),
    ("RESIDENT_NWG", "-4", -4), ("RESIDENT_NWG", "100000", 100000),       # (clamped to the plan's CUs where it is used)
    ("SPLIT", "0", 0), ("SPLIT", "5", 1), ("DENSE_SYMV", "0", 0), ("DENSE_CHOL", "0", 0), ("DENSE_CHOL", "1", 1),
    ("RESIDENT_FINE", "0", 0), ("RESIDENT_INJECT", "4", 4), ("TRACE_MAPS", "maps.txt", len("maps.txt")),
])
def test_one_switch_set(clean_env, name, text, want):
    before = values()
    clean_env.setenv("OSQP_AMD_" + name, text)
    after = values()
    assert after[name] == want
    assert {k: x for k, x in after.items() if k != name} == {k: x for k, x in before.items() if k != name}


def test_unset_is_a_value_of_its_own_where_the_problem_decides(clean_env):
    v = values()
    assert all(v[k] == UNSET for k in PROBLEM_DEPENDENT)
    assert v["RESIDENT_NWG"] == 0          # (its "unset" is the value 0: the grid sized to the problem)
    for k in PROBLEM_DEPENDENT:             # and no value that can be set collides with it
        for text in ("0", "-1", "-7"):
            clean_env.setenv("OSQP_AMD_" + k, text)
            assert values()[k] == (UNSET if k == "CHUNK" else 1 if k == "FIN_GRID" else float(text != "0"))
            clean_env.delenv("OSQP_AMD_" + k)


def test_defaults_of_the_python_restatement():
    from tests._kkt_instance_cases import SWITCH_DEFAULTS
    assert set(SWITCH_DEFAULTS) == {"OSQP_AMD_" + k for k in ("RESIDENT_MIN_N", "DENSE_SMALL", "DENSE_DIRECT", "ELIM", "RESIDENT",
                                                               "RESIDENT_BLOCKS", "BLOCK_DIRECT")}
    text = {r[0]: r[2] for r in table()}
    for k, d in SWITCH_DEFAULTS.items():
        assert float(text[k]) == d, k


def _tokens(path):
    with open(path) as f:
        return set(re.findall(r"OSQP_AMD_[A-Z0-9_]+", f.read()))


def test_no_unknown_switch_anywhere():
    known = {r[0] for r in table()} | other_library_names() | ALLOWED
    files = [p for pat in ("tests/*.py", "tools/*.py", "tools/*.sh", "osqp_amd/*.py") for p in glob.glob(os.path.join(ROOT, pat))]
    files += [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    assert len(files) > 50
    unknown = {}
    for p in files:
        for t in _tokens(p):
            if t not in known and not t.startswith(ALLOWED_PREFIX):
                unknown.setdefault(t, []).append(os.path.relpath(p, ROOT))
    assert not unknown, unknown


def test_integration_md_names_every_engine_switch_once():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    section = doc[doc.index("## F. Environment variables"):]
    section = section[:section.index("\nProfiling with rocprofv3")]
    rows = [ln.split("|") for ln in section.splitlines() if ln.startswith("| `")]
    para = section[section.index("Diagnostics / tuning"):]
    named, defaults = [], {}
    for cells in rows:
        names = re.findall(r"OSQP_AMD_[A-Z0-9_]+", cells[1])
        named += names
        if len(names) == 1:
            defaults[names[0]] = cells[2].strip()
    named += re.findall(r"OSQP_AMD_[A-Z0-9_]+", para)
    tab = {r[0]: r for r in table()}
    engine = [n for n in named if n not in other_library_names()]
    assert sorted(engine) == sorted(tab), (set(tab) - set(engine), set(engine) - set(tab), [n for n in set(engine) if engine.count(n) > 1])
    plain = 0
    for name, text in defaults.items():
        if name in tab and re.fullmatch(r"-?[0-9.]+(e-?[0-9]+)?", text):
            assert not tab[name][3] and float(text) == float(tab[name][2]), name
            plain += 1
    assert plain >= 20
