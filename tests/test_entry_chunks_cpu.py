"""How sgpu_batch_search cuts a call into launches once the number of chunks depends on the size of the call (abi.cpp
chunk_jobs / chunk_bounds / call_segments, through the debug exports; no GPU needed): the launches are contiguous, in
order, non-empty, cover [0, nq) exactly once, and none exceeds the 16384 queries a lane's arena and a launch plan are sized
for - up to eight per segment through sgpu_debug_chunk_bounds (which describes ONE segment: at most 8 x 16384 queries
keep the bound there), any number of queries through sgpu_debug_call_bounds (segments one after the other)."""
import ctypes

from seismic_amd import _native

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
