"""A call of sgpu_batch_search cut in chunks: who plans which chunk, and that it never shows in the rows.

Chunk 0 of a multi-chunk call goes out unplanned (input order), every later chunk is planned by the calling thread while
the GPU searches the chunk before it (SGPU_CHUNK_PLAN=device: on the device, the rule before; SGPU_DEVICE_PLAN=0: the host
plans everything). Whatever the cut and whoever plans, the rows are those of a one-chunk call of the same queries and the
oracle's, bit for bit: scores as u32, ids and counts exact.

SGPU_CHUNK_MIN / SGPU_CHUNK_MAX are read once per process, so every cut runs in a child process of its own (this file run as
a script); the knobs that are read per call are flipped inside a child. The children run once per session (module
fixture): one index, built and saved by the parent, and one oracle result per query set are shared by all tests.
Run with `-m gpu` on an MI355X."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DIM, N_DOCS, HF = 3000, 20000, 0.9
# boundaries of the 2-, 3- and 4-way cuts (floor(nq * j / n)); a query set has an empty query ON some of them and right
# BEFORE the others (the chunk then starts with the query after an empty one: rebased offsets off[q - q0]), and an empty
# last query
SETS = {"q601": 601, "q1021": 1021, "q1100": 1100}
CUTS = {"c2": 2, "c3": 3, "c4": 4}
MODES = {"host": {}, "device": {"SGPU_CHUNK_PLAN": "device"}, "allhost": {"SGPU_DEVICE_PLAN": "0"}}
# (k, query_cut, first_sorted, filtered) of the variants searched on q1021; "base" is what every set is searched with
VARIANTS = {"base": (10, 4, False, False), "k1": (1, 4, False, False), "k100": (100, 4, False, False),
            "sorted": (10, 4, True, False), "cut20": (10, 20, False, False), "filtered": (10, 4, False, True)}


def boundaries(nq):
    return sorted({nq * j // n for n in (2, 3, 4) for j in range(1, n)})


def make_queries(seed, nq):
    from util import random_queries
    off, c, v = random_queries(seed, nq, DIM, 3, 30)
    empty = {nq - 1}
    for i, b in enumerate(boundaries(nq)):
        empty.add(b if i % 2 == 0 else b - 1)
    keep = np.ones(len(c), bool)
    lens = np.diff(off.astype(np.int64))
    for q in empty:
        keep[int(off[q]):int(off[q + 1])] = False
        lens[q] = 0
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return new_off, np.ascontiguousarray(c[keep]), np.ascontiguousarray(v[keep])


def allowed_docs():
    return np.random.default_rng(7).random(N_DOCS) < 0.4


# ---------------------------------------------------------------------------------------------------------------
# the child: one process per (SGPU_CHUNK_MIN, SGPU_CHUNK_MAX); argv = work directory, name of the cut
def child(work, cut_name):
    from seismic_amd import _native
    ix = _native.NativeIndex.load(os.path.join(work, "index.idx"))
    ix.upload(0)
    L = _native.lib()
    qs = {name: tuple(np.load(os.path.join(work, name + ".npz"))[k] for k in ("off", "c", "v")) for name in SETS}
    flt = ix.make_filter(allowed_docs())
    out = {}

    def search(q, variant="base", env=None):
        k, cut, fs, filtered = VARIANTS[variant]
        for n_, v_ in (env or {}).items():
            os.environ[n_] = v_
        try:
            return ix.batch_search(*q, k, cut, HF, fs, filter=flt if filtered else None)
        finally:
            for n_ in (env or {}):
                del os.environ[n_]

    def keep(tag, rows):
        out[tag + ".s"], out[tag + ".i"], out[tag + ".n"] = rows[0].view(np.uint32).copy(), rows[1].copy(), rows[2].copy()

    def same(a, b):
        return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))

    search(qs["q1021"])   # (the first call's host plans tell what this index needs at query_cut 4: the device plans from here on)
    for name in SETS:
        for mode, env in MODES.items():
            keep("%s.base.%s" % (name, mode), search(qs[name], "base", env))
    for variant in VARIANTS:
        if variant != "base":
            keep("q1021.%s.host" % variant, search(qs["q1021"], variant))
    base = search(qs["q1021"])

    # who planned the chunks of the last call (a lone caller takes lanes 0, 1, ...), and the order a later chunk went down with
    if cut_name != "one":
        sig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.sgpu_debug_plan.argtypes = sig
        L.sgpu_debug_device_plan.argtypes = sig
        L.sgpu_debug_lane_chunk.restype = ctypes.c_uint32
        L.sgpu_debug_lane_chunk.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        off, c, v = qs["q1021"]
        for mode, env in MODES.items():
            search(qs["q1021"], "base", env)
            lanes = []
            for lane in range(8):
                info, order = np.zeros(4, np.uint32), np.zeros(2048, np.uint32)
                if not L.sgpu_debug_lane_chunk(ix.h, lane, p(info), p(order), len(order)):
                    continue
                nq, q0 = int(info[0]), int(info[1])
                if q0 + nq > len(off) - 1:   # (a lane this call did not take: what it holds is an earlier call's)
                    continue
                co = np.ascontiguousarray(off[q0:q0 + nq + 1] - off[q0])
                cc, cv = c[int(off[q0]):int(off[q0 + nq])], v[int(off[q0]):int(off[q0 + nq])]
                ho, do, x3 = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32), np.zeros(3, np.uint32)
                assert L.sgpu_debug_plan(ix.h, p(co), p(cc), p(cv), nq, 4, p(ho), p(x3)) == 0
                assert L.sgpu_debug_device_plan(ix.h, p(co), p(cc), p(cv), nq, 4, p(do), p(x3)) == 0
                lanes.append([nq, q0, int(info[2]), int(info[3]),
                              bool(np.array_equal(order[:nq], ho)), bool(np.array_equal(ho, do))])
            out["lanes." + mode] = np.array(lanes, np.int64)

    # an invalid component in a LATER chunk (the last query with components): SGPU_EINVAL naming the query, every launched
    # chunk waited for - the next call on the same index returns the rows
    off, c, v = qs["q1021"]
    last = max(q for q in range(len(off) - 1) if off[q + 1] > off[q])
    bad = c.copy()
    bad[int(off[last + 1]) - 1] = DIM + 3
    try:
        ix.batch_search(off, bad, v, 10, 4, HF, False)
        out["bad"] = np.array([0])
    except _native.SeismicHipError as e:
        out["bad"] = np.array([1 if e.status == 1 and ("query %d" % last) in str(e) else 2])   # (1: SGPU_EINVAL)
    out["after_bad"] = np.array([same(search(qs["q1021"]), base)])

    # fewer free lanes than chunks wanted: three request threads on multi-chunk calls hold each other's lanes
    ok = []

    def worker():
        ok.append(all(same(search(qs["q1021"]), base) for _ in range(3)))
    th = [threading.Thread(target=worker) for _ in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    out["threads"] = np.array([len(ok) == 3 and all(ok)])
    np.savez(os.path.join(work, "rows_%s.npz" % cut_name), **out)


# the child of the rule: SGPU_CHUNK_MIN / SGPU_CHUNK_MAX unset, so the library cuts by its own rule (call_cut.cpp: cut_rule).
# The sizes at which the 600 and the 1300 rule flip between one launch and two.
RULE_SIZES = (1199, 1200, 2599, 2600)


def rule_child(work):
    """Per size, on a replica uploaded afresh (its lanes have served nothing): the first call - nothing has told the device
    what the index needs, the host plans - and a second one, each from this one thread with nothing else on the replica.
    Recorded per call: what every pool lane reports (sgpu_debug_lane_chunk) and, for device_plans 0 and 1, what
    sgpu_debug_cut_rule(shared=0, device_plans) and cut_segment under it (sgpu_debug_chunk_bounds) say."""
    from seismic_amd import _native
    from util import random_queries
    ix = _native.NativeIndex.load(os.path.join(work, "index.idx"))
    L = _native.lib()
    L.sgpu_debug_lane_chunk.restype = ctypes.c_uint32
    L.sgpu_debug_lane_chunk.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    L.sgpu_debug_chunk_bounds.restype = ctypes.c_uint32
    L.sgpu_debug_chunk_bounds.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    out = {}
    for nq in RULE_SIZES:
        q = random_queries(200 + nq, nq, DIM, 3, 30)
        for dp in (0, 1):
            chunk_min, chunk_max = _native.debug_cut_rule(0, dp)
            bounds = np.zeros(16, np.uint32)
            n = L.sgpu_debug_chunk_bounds(nq, chunk_min, chunk_max, 8, p(bounds))
            out["want.%d.%d" % (nq, dp)] = np.concatenate([[chunk_min, chunk_max], bounds[:2 * n]]).astype(np.int64)
        ix.upload(0)
        for call in (0, 1):
            ix.batch_search(*q, 10, 4, HF, False)
            lanes = []
            for lane in range(8):
                info = np.zeros(4, np.uint32)
                if L.sgpu_debug_lane_chunk(ix.h, lane, p(info), None, 0):
                    lanes.append([lane] + [int(x) for x in info])
            out["lanes.%d.%d" % (nq, call)] = np.array(lanes, np.int64).reshape(-1, 5)
    np.savez(os.path.join(work, "rows_rule.npz"), **out)


if __name__ == "__main__":
    if sys.argv[2] == "rule":
        rule_child(sys.argv[1])
    else:
        child(sys.argv[1], sys.argv[2])
    sys.exit(0)

import pytest  # noqa: E402

import orc  # noqa: E402
from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig, IndexDesc  # noqa: E402
from util import random_dataset  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The index, the query sets, the oracle's rows and the rows of every child (one chunk; 2, 3, 4 chunks)."""
    work = str(tmp_path_factory.mktemp("entry_chunks"))
    off, comps, vals = random_dataset(91, N_DOCS, DIM, nnz_lo=8, nnz_hi=90)
    ix = _native.NativeIndex.build(2, DIM, off, comps, vals,
                                   BuildConfig.defaults(n_postings=300, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0))
    ix.save(os.path.join(work, "index.idx"))
    qs = {}
    for i, (name, nq) in enumerate(SETS.items()):
        qs[name] = make_queries(92 + i, nq)
        np.savez(os.path.join(work, name + ".npz"), off=qs[name][0], c=qs[name][1], v=qs[name][2])
    rows = {}
    for cut_name, n in [("one", 0)] + list(CUTS.items()):
        env = dict(os.environ, SGPU_TEST_HOOKS="1", SGPU_CHUNK_MIN="150" if n else "0")   # (150: also 601 queries are cut in four)
        env.pop("SGPU_CHUNK_PLAN", None)
        env.pop("SGPU_DEVICE_PLAN", None)
        if n:
            env["SGPU_CHUNK_MAX"] = str(n)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), work, cut_name], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (cut_name, r.stdout[-2000:], r.stderr[-4000:])
        rows[cut_name] = dict(np.load(os.path.join(work, "rows_%s.npz" % cut_name)))
    return {"ix": ix, "qs": qs, "rows": rows, "oracle": {}, "work": work}


class _FilteredDesc:
    """The descriptor with the postings of documents outside `allowed` deleted (as tests/test_gpu_filter.py builds it)."""

    def __init__(self, desc, allowed):
        a = orc.desc_arrays(desc)
        keep = allowed[a["post_doc"]]
        cum = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)]).astype(np.uint64)
        self.bps = np.ascontiguousarray(cum[a["block_post_start"].astype(np.int64)], np.uint64)
        self.post_doc = np.ascontiguousarray(a["post_doc"][keep], np.uint32)
        self.desc = IndexDesc()
        ctypes.memmove(ctypes.byref(self.desc), ctypes.byref(desc), ctypes.sizeof(IndexDesc))
        self.desc.n_postings = len(self.post_doc)
        self.desc.block_post_start = self.bps.ctypes.data_as(type(desc.block_post_start))
        self.desc.post_doc = (self.post_doc if len(self.post_doc) else np.zeros(1, np.uint32)).ctypes.data_as(type(desc.post_doc))


def _oracle(runs, name, variant):
    """The oracle's rows of a query set, computed once and shared."""
    key = (name, variant)
    if key not in runs["oracle"]:
        k, cut, fs, filtered = VARIANTS[variant]
        desc = runs["ix"].desc
        if filtered:
            fd = runs["oracle"].setdefault("fd", _FilteredDesc(desc, allowed_docs()))
            desc = fd.desc
        runs["oracle"][key] = orc.batch_search(desc, *runs["qs"][name], k, cut, HF, fs)[:3]
    return runs["oracle"][key]


def _rows(runs, cut_name, tag):
    r = runs["rows"][cut_name]
    return r[tag + ".s"], r[tag + ".i"], r[tag + ".n"]


def _assert_same(got, want, what):
    gs, gi, gn = got
    ws, wi, wn = want
    assert np.array_equal(gn, wn), (what, np.flatnonzero(gn != wn)[:5])
    for q in range(len(gn)):
        n = int(gn[q])
        assert np.array_equal(gi[q, :n], wi[q, :n]), (what, q)
        assert np.array_equal(gs[q, :n], ws[q, :n].view(np.uint32)), (what, q)


def test_the_query_sets_put_empty_queries_on_and_before_the_boundaries(runs):
    for name, nq in SETS.items():
        off = runs["qs"][name][0]
        lens = np.diff(off.astype(np.int64))
        assert len(lens) == nq and lens[nq - 1] == 0
        on = [b for b in boundaries(nq) if lens[b] == 0]
        before = [b for b in boundaries(nq) if lens[b - 1] == 0 and lens[b] > 0]
        assert on and before and len(on) + len(before) == len(boundaries(nq)), (name, on, before)


@pytest.mark.parametrize("name", list(SETS))
def test_one_chunk_rows_are_the_oracles(runs, name):
    for mode in MODES:
        _assert_same(_rows(runs, "one", "%s.base.%s" % (name, mode)), _oracle(runs, name, "base"), (name, mode))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cut_name", list(CUTS))
@pytest.mark.parametrize("name", list(SETS))
def test_chunked_rows_are_the_one_chunk_rows_and_the_oracles(runs, name, cut_name, mode):
    """2, 3 and 4 chunks, nq not divisible by the count, boundaries on and right after empty queries, an empty last query;
    later chunks planned by the host (default), by the device, everything by the host."""
    got = _rows(runs, cut_name, "%s.base.%s" % (name, mode))
    one = _rows(runs, "one", "%s.base.host" % name)
    for a, b in zip(got, one):
        assert np.array_equal(a, b), (name, cut_name, mode)
    _assert_same(got, _oracle(runs, name, "base"), (name, cut_name, mode))


@pytest.mark.parametrize("cut_name", list(CUTS))
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "base"])
def test_k_sorted_first_list_large_cut_and_filter_are_unchanged_by_the_cut(runs, variant, cut_name):
    """k = 1 and k = 100; first_sorted and query_cut > 16 (host-plan-only configurations); a filtered call."""
    got = _rows(runs, cut_name, "q1021.%s.host" % variant)
    one = _rows(runs, "one", "q1021.%s.host" % variant)
    for a, b in zip(got, one):
        assert np.array_equal(a, b), (variant, cut_name)
    _assert_same(got, _oracle(runs, "q1021", variant), (variant, cut_name))


@pytest.mark.parametrize("cut_name", list(CUTS))
def test_who_plans_which_chunk(runs, cut_name):
    """Chunk 0 of a call whose chunks the device could plan goes out unplanned; a later chunk is planned by the host and goes
    down with the order sgpu_debug_plan and sgpu_debug_device_plan give for its queries; SGPU_CHUNK_PLAN=device hands the
    later chunks to the device, SGPU_DEVICE_PLAN=0 everything to the host."""
    n = CUTS[cut_name]
    nq = SETS["q1021"]
    for mode in MODES:
        lanes = {int(r[1]): r for r in runs["rows"][cut_name]["lanes." + mode]}
        for j in range(n):
            q0, q1 = nq * j // n, nq * (j + 1) // n
            device_size = q1 - q0 >= 256   # (the device plans launches of at least 256 queries: kDevicePlanMinQueries)
            assert q0 in lanes and int(lanes[q0][0]) == q1 - q0, (cut_name, mode, j, sorted(lanes))
            _, _, planner, cut, order_is_host_plan, host_is_device = (int(x) for x in lanes[q0])
            assert cut == 4 and host_is_device
            if mode == "allhost" or not device_size:
                want = 0
            elif j == 0:
                want = 2
            elif mode == "host":
                want = 0
            else:
                want = 1 if j == n - 1 else 2   # (the rule before: a chunk followed by another of its call is not planned)
            assert planner == want, (cut_name, mode, j, planner, want)
            if planner == 0:
                assert order_is_host_plan, (cut_name, mode, j)


@pytest.mark.parametrize("cut_name", list(CUTS))
def test_an_invalid_component_in_a_later_chunk_fails_the_call_and_not_the_next(runs, cut_name):
    assert int(runs["rows"][cut_name]["bad"][0]) == 1
    assert bool(runs["rows"][cut_name]["after_bad"][0])


@pytest.mark.parametrize("cut_name", list(CUTS))
def test_three_request_threads_share_the_lanes(runs, cut_name):
    assert bool(runs["rows"][cut_name]["threads"][0])


def test_the_library_cuts_by_the_rule_the_hooks_describe(runs):
    """SGPU_CHUNK_MIN / SGPU_CHUNK_MAX unset, one request thread on an idle replica (shared = 0), 1199 / 1200 / 2599 / 2600
    queries - where the 600 and the 1300 rule flip between one launch and two: the pool lanes that served a call, and their
    [q0, q1), are cut_segment's under sgpu_debug_cut_rule(0, device_plans). device_plans is read off the lanes, not guessed:
    0 where every chunk of the call was planned by the host (the first call on a fresh replica: nothing has told the device
    what the index needs), 1 where a chunk went out planned by the device or unplanned. info4 says who planned a chunk, not
    which rule cut the call; a lone caller takes the pool's lanes in order, so lane 0 always holds this call's first chunk,
    and a cut into another number of chunks than the rule's shows in that chunk's size. On the fresh replica the lanes that
    report anything at all are exactly the call's."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SGPU_CHUNK_") and k != "SGPU_DEVICE_PLAN"}
    env["SGPU_TEST_HOOKS"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), runs["work"], "rule"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rows = dict(np.load(os.path.join(runs["work"], "rows_rule.npz")))
    for nq in RULE_SIZES:
        # the rule itself, as tests/test_entry_chunks_cpu.py pins it, and the launches it leads to at these sizes
        assert list(rows["want.%d.0" % nq][:2]) == [600, 4] and list(rows["want.%d.1" % nq][:2]) == [1300, 2]
        assert len(rows["want.%d.0" % nq]) // 2 - 1 == {1199: 1, 1200: 2, 2599: 4, 2600: 4}[nq]   # (at least 600 each, up to four)
        assert len(rows["want.%d.1" % nq]) // 2 - 1 == {1199: 1, 1200: 1, 2599: 1, 2600: 2}[nq]   # (at least 1300 each, up to two)
        for call in (0, 1):
            lanes = rows["lanes.%d.%d" % (nq, call)]
            print("nq %d call %d: lanes (lane, queries, first query, planner, query_cut) %s" % (nq, call, lanes.tolist()))
            assert len(lanes) and lanes[0][0] == 0
            dp = int(lanes[0][3] != 0)   # (who planned the call's first chunk: the host plans it only where the device cannot)
            if call == 0:
                assert dp == 0, (nq, lanes.tolist())
            want = rows["want.%d.%d" % (nq, dp)][2:].reshape(-1, 2)
            got = [(int(q0), int(q0 + n_)) for _, n_, q0, _, _ in lanes[:len(want)]]
            assert got == [tuple(int(x) for x in w) for w in want], (nq, call, dp, lanes.tolist(), want.tolist())
            assert [int(x) for x in lanes[:len(want), 0]] == list(range(len(want)))
            if call == 0:
                assert len(lanes) == len(want), (nq, lanes.tolist())   # (no other lane has served anything)
