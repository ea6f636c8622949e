"""How sgpu_batch_search cuts a call into launches once the number of chunks depends on the size of the call
(seismic_amd/csrc/call_cut.cpp: cut_rule / cut_segment / call_segments, through the debug exports; no GPU needed): the launches are contiguous, in
order, non-empty, cover [0, nq) exactly once, and none exceeds the 16384 queries a lane's arena and a launch plan are sized
for - up to eight per segment through sgpu_debug_chunk_bounds (which describes ONE segment: at most 8 x 16384 queries
keep the bound there), any number of queries through sgpu_debug_call_bounds (segments one after the other).

The rule that picks chunk_min and chunk_max (sgpu_debug_cut_rule) is checked row by row in child processes - the knobs are
read once per process -, and both bounds hooks against tests/golden/call_cut_bounds.json: the answers of the library as it
was before the cut moved out of abi.cpp, recorded by running this file as a script against that build
(SGPU_LIB=<its libseismic_hip.so> SGPU_TEST_HOOKS=1 python tests/test_entry_chunks_cpu.py record)."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from seismic_amd import _native  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "call_cut_bounds.json")

CHUNK_QUERIES_MAX = 16384   # kChunkQueriesMax (seismic_amd/csrc/common.hpp) = kDevicePlanMaxQueries


def _lib():
    L = ctypes.CDLL(_native.LIB_PATH)
    L.sgpu_debug_chunk_bounds.restype = ctypes.c_uint32
    L.sgpu_debug_chunk_bounds.argtypes = [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint32)]
    L.sgpu_debug_call_bounds.restype = ctypes.c_uint32
    L.sgpu_debug_call_bounds.argtypes = [ctypes.c_uint32] * 5 + [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    return L


SIZES = [1, 2, 599, 1300, 2599, 2600, 10000, 16384, 16385, 32768, 32769, 49153, 65536, 65537, 100003, 131072, 131073, 150000,
         199999, 200000]


def _check(b, n, nq, limit):
    assert n >= 1 and b[0] == 0 and b[2 * n - 1] == nq
    for j in range(n):
        assert b[2 * j] < b[2 * j + 1] or nq == 0
        assert b[2 * j + 1] - b[2 * j] <= limit, (nq, n, j, b[2 * j], b[2 * j + 1])
        if j:
            assert b[2 * j] == b[2 * j - 1]


def test_no_chunk_of_a_segment_exceeds_what_a_lane_was_sized_for():
    L = _lib()
    bounds = (ctypes.c_uint32 * 16)()
    for nq in SIZES:
        for chunk_min, chunk_max in ((1300, 2), (600, 4), (600, 2), (4000, 2)):
            n = L.sgpu_debug_chunk_bounds(nq, chunk_min, chunk_max, 8, bounds)
            assert 1 <= n <= 8
            if nq <= 8 * CHUNK_QUERIES_MAX:
                _check(list(bounds), n, nq, CHUNK_QUERIES_MAX)
                assert n >= -(-nq // CHUNK_QUERIES_MAX)
    # the defaults of a call whose chunks the device could plan: 10 000 queries -> two launches, 2500 -> one, 40 000 -> three
    assert L.sgpu_debug_chunk_bounds(10000, 1300, 2, 8, bounds) == 2 and bounds[1] == 5000
    assert L.sgpu_debug_chunk_bounds(2500, 1300, 2, 8, bounds) == 1
    assert L.sgpu_debug_chunk_bounds(40000, 1300, 2, 8, bounds) == 3
    # SGPU_CHUNK_MIN=0 still means: never cut a call
    assert L.sgpu_debug_chunk_bounds(40000, 0, 2, 8, bounds) == 1


def test_a_call_of_any_size_is_cut_within_the_bound():
    L = _lib()
    cap = 64
    bounds = (ctypes.c_uint32 * (2 * cap))()
    for nq in SIZES + [1000003]:
        for chunk_min, chunk_max in ((1300, 2), (600, 4)):
            n = L.sgpu_debug_call_bounds(nq, chunk_min, chunk_max, 8, 0, bounds, cap)
            assert n <= cap
            _check(list(bounds), n, nq, CHUNK_QUERIES_MAX)
    # fewer free lanes than chunks wanted: the cut follows the lanes (the bound is then the lanes' to give)
    n = L.sgpu_debug_call_bounds(200000, 1300, 2, 3, 0, bounds, cap)
    _check(list(bounds), n, 200000, 200000)
    assert n == 6   # two segments of three launches


def test_a_smaller_first_chunk_keeps_the_cover():
    L = _lib()
    bounds = (ctypes.c_uint32 * 32)()
    for nq in (601, 1021, 10000):
        for n_max in (2, 3, 4):
            for pm in (150, 300, 500, 999):
                n = L.sgpu_debug_call_bounds(nq, 100, n_max, 8, pm, bounds, 16)
                assert n == n_max
                _check(list(bounds), n, nq, nq)
    assert L.sgpu_debug_call_bounds(10000, 1300, 2, 8, 300, bounds, 16) == 2 and bounds[1] == 3000


# ---- the hooks against the library before the cut became call_cut.cpp ------------------------------------------------
PAIRS = ((1300, 2), (600, 4), (600, 2), (4000, 2))


def grid_answers(L):
    """{"nq chunk_min chunk_max lanes_free first_pm": [launches of sgpu_debug_chunk_bounds (first_pm 0 only), launches of
    sgpu_debug_call_bounds]}, each a flat list q0, q1, q0, q1, ..."""
    out = {}
    b8, cap = (ctypes.c_uint32 * 16)(), 64
    bc = (ctypes.c_uint32 * (2 * cap))()
    for nq in SIZES:
        for chunk_min, chunk_max in PAIRS:
            for lanes in (1, 3, 8):
                for pm in (0, 300):
                    n = L.sgpu_debug_call_bounds(nq, chunk_min, chunk_max, lanes, pm, bc, cap)
                    assert 1 <= n <= cap
                    row = [None, list(bc[:2 * n])]
                    if pm == 0:
                        n = L.sgpu_debug_chunk_bounds(nq, chunk_min, chunk_max, lanes, b8)
                        assert 1 <= n <= 8
                        row[0] = list(b8[:2 * n])
                    out["%d %d %d %d %d" % (nq, chunk_min, chunk_max, lanes, pm)] = row
    return out


def test_the_bounds_hooks_answer_as_the_library_did_before_the_cut_moved():
    want = json.load(open(GOLDEN))
    got = grid_answers(_lib())
    assert sorted(got) == sorted(want) and len(got) == len(SIZES) * len(PAIRS) * 3 * 2
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])


# ---- the rule: one child process per row (SGPU_CHUNK_MIN / SGPU_CHUNK_MAX are read once per process) -------------------
_RULE_CHILD = """
import ctypes, json, sys
import numpy as np
from seismic_amd import _native
L = ctypes.CDLL(_native.LIB_PATH)
L.sgpu_last_error.restype = ctypes.c_char_p
L.sgpu_debug_cut_rule.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
rows = []
for shared, dp in ((0, 0), (1, 0), (0, 1), (1, 1)):
    out = np.full(2, 77, np.uint32)
    st = L.sgpu_debug_cut_rule(shared, dp, out.ctypes.data_as(ctypes.c_void_p))
    rows.append([int(st), int(out[0]), int(out[1]), L.sgpu_last_error().decode() if st else ""])
print(json.dumps(rows))
"""


def _rule(**env):
    """[status, chunk_min, chunk_max, message] of sgpu_debug_cut_rule for (shared, device_plans) = (0,0) (1,0) (0,1) (1,1) in a
    fresh process whose SGPU_CHUNK_* are exactly `env`."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("SGPU_CHUNK_")}
    e["SGPU_TEST_HOOKS"] = "1"
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE)] + [p for p in e.get("PYTHONPATH", "").split(os.pathsep) if p])
    r = subprocess.run([sys.executable, "-c", _RULE_CHILD], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_the_rule_without_knobs():
    assert [r[:3] for r in _rule()] == [[0, 600, 4], [0, 600, 2], [0, 1300, 2], [0, 1300, 2]]


def test_chunk_min_overrides_the_rule_and_zero_stays_zero():
    assert [r[:3] for r in _rule(SGPU_CHUNK_MIN="150")] == [[0, 150, 4], [0, 150, 2], [0, 150, 2], [0, 150, 2]]
    assert [r[:3] for r in _rule(SGPU_CHUNK_MIN="0")] == [[0, 0, 4], [0, 0, 2], [0, 0, 2], [0, 0, 2]]


def test_chunk_max_overrides_the_rule_and_is_clamped_to_eight():
    assert [r[:3] for r in _rule(SGPU_CHUNK_MAX="3")] == [[0, 600, 3], [0, 600, 3], [0, 1300, 3], [0, 1300, 3]]
    assert [r[:3] for r in _rule(SGPU_CHUNK_MAX="99")] == [[0, 600, 8], [0, 600, 8], [0, 1300, 8], [0, 1300, 8]]


def test_the_rule_hook_is_inert_without_the_switch():
    for st, chunk_min, chunk_max, msg in _rule(SGPU_TEST_HOOKS="0"):
        assert st == 1 and (chunk_min, chunk_max) == (77, 77)   # (1: SGPU_EINVAL; out2 untouched)
        assert "sgpu_debug_cut_rule is a test hook" in msg


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    json.dump(grid_answers(_lib()), open(GOLDEN, "w"), separators=(",", ":"), sort_keys=True)
    print("wrote", GOLDEN)
