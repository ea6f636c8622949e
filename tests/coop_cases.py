"""Seeded inputs for the tests of the cooperative search rounds (seismic_amd/csrc/search_coop.inc) at the
edges of their board and their replay (test_coop_cases_cpu.py, test_gpu_coop_edges.py), and a RESTATEMENT of the forced
schedule in numpy. TEST INFRASTRUCTURE, pure numpy apart from the index build and the oracle's f32 scores.

The block-size technique is stream_cases.py's (imported, not copied): centroid_fraction 1e-6 makes one block per list,
centroid_fraction 1.0 with two signature components per document makes blocks of one posting, values are multiples of
1/64 so binary16, fixed-u8 and DotVByte hold the same numbers.

Why a forced launch can be restated. Under SGPU_COOP=force idle_min and idle_ratio are 0: an owner goes wide from its own
state alone. Which workgroup takes which chunk does not change which documents are scored, and the owner ranks the
candidates by key (position << 16 | posting) before it replays them. So the sequence of local rounds, wide rounds and
fallbacks of a query, every round's start (list, position), its n_pos, its starting threshold, its candidate count nc and
the number of documents scored (work counter [7] of sgpu_batch_fetch_stats) are a function of the input and the knobs.
schedule() is that function, for these cases only: every run sets SGPU_COOP_MIN_ITEMS=0 and SGPU_ITEMS_INIT, so the local
part is the first local round(s) that fill the heap (every block live, a prefix of blocks by the item budget, the budget
doubling while the heap is not full), then wide rounds: a first one of first_reach positions, a second one over the rest
of the list group; a round with nc > max_cand, with an unkeyable posting or with n_pos == 0 falls back, and the query
stays local from where that round BEGAN. Thresholds and scores are the oracle's f32 values (orc.score_doc,
orc.summary_distances), never the device's. After a fallback the local rounds score every posting that is left when
heap_factor <= 0 (nothing is skipped); for heap_factor > 0 the blocks a local round skips depend on the threshold at the
ROUND's start, which the restatement does not model: it then gives the bounds [blocks live at their own start, every
posting left]. kNN refinement runs behind the rounds: the restatement stops in front of it (its rows are then not
compared, and counter [7] is bounded by at most n * n_knn more documents).

Every run names the edge it is there for (Run.edge; the lists in _units_runs and _blocks), and check() proves each reached.

NOT reachable, and why:
  n_pos > max_pos        max_pos is the dots capacity, and a list group only holds lists whose blocks fit that capacity.
  give-up codes 1, 2, 3  need a wait that runs out or control words of another round: no test stalls a role or forces a wait.
  a fallback that leaves pos >= nb   a failed round puts (list, position) back to where it began, which lies inside a list
                         (the round loop enters a wide round only while pos < nb; an accepted first round that ended exactly
                         at a list's end hands the NEXT list to the second round, the `wl != l` resume). The nearest reachable
                         edge is a second round that began in the list the first one began in (run `second_same_list`).
"""
import contextlib
import functools
import os

import numpy as np

import orc
import stream_cases as SC
from seismic_amd import _native

WINDOW = 64                 # candidates per replay window of the owner
BLOCKS = SC.BLOCKS          # SGPU_BLOCK
FACTORS = SC.FACTORS
KS = (1, 64, 65, 128, 129, 256)
K_PLAIN = 257               # no cooperative symbol: the plain variant
KEY_MAX = 0xffff            # posting index within a block that a candidate key still holds
READINGS = ("overflow_ge", "resume_at_end", "decided_per_window", "no_heap_contains", "first_unbounded", "order_every_list")


class Run(SC.Run):
    """stream_cases.Run + the edge the run is there for and the mode: "force" (deterministic, counter [7] compared) or
    "auto" (SGPU_COOP unset: timing decides who helps, rows only)."""

    def __init__(self, name, edge, queries, k, cut, hf, mode="force", init=64, **kw):
        env = dict(kw.pop("env", None) or {})
        super().__init__(name, queries, k, cut, hf, env=env, **kw)
        self.edge, self.mode, self.init = edge, mode, init


class CoopCase(SC.StreamCase):
    pass


def knob_env(case, run, block):
    """The environment a run is launched under."""
    env = dict(SGPU_COOP_MIN_ITEMS="0", SGPU_ITEMS_INIT=str(run.init), SGPU_BLOCK=str(block))
    if run.mode == "force":
        env["SGPU_COOP"] = "force"
    if SC.FORMS[case.form] == (4, 0) and "SGPU_FORCE_HASH" not in run.env:
        env["SGPU_NO_HASH"] = "1"      # (unforced runs keep the other layouts; the hashed lookup has test_gpu_hash_lookup.py)
    env.update(run.env)
    return env


@contextlib.contextmanager
def knobs(env):
    """The SGPU_* environment of a launch, put back afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def hook(case, ix, run, block, **chip):
    """sgpu_debug_launch_config for a run under its knobs (no device)."""
    Q = case.batch(run)
    with knobs(knob_env(case, run, block)):
        return _native.debug_launch_config(heap_factor=run.hf, **dict(SC.plan_facts(case, ix, run, Q), **chip))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.float32(x)


class _Heap:
    """RegHeap: best first by (score descending, document ascending), at most k entries."""

    def __init__(self, k):
        self.k, self.e = k, []

    @property
    def full(self):
        return len(self.e) == self.k

    @property
    def thr(self):
        return self.e[self.k - 1][0]

    def contains(self, doc):
        return any(d == doc for _, d in self.e)

    def insert(self, s, doc):
        rank = sum(1 for (x, d) in self.e if x > s or (x == s and d < doc))
        self.e.insert(rank, (s, doc))
        del self.e[self.k:]


class _Lists:
    """What a query walks: per list its blocks in index order (first posting, count), the oracle's f32 summary dots and
    the oracle's f32 scores of the documents met."""

    def __init__(self, case, desc, arrays, qname, cut):
        self.desc, self.a = desc, arrays
        self.qc, self.qv = case.queries[qname]
        order = np.lexsort((self.qc, -self.qv.astype(np.float64)))          # descending weight, ties by ascending component
        self.lists = [int(self.qc[i]) for i in order[:cut]]
        lbs, bps = arrays["list_block_start"].astype(np.int64), arrays["block_post_start"].astype(np.int64)
        self.b0 = [int(lbs[c]) for c in self.lists]
        self.nb = [int(lbs[c + 1] - lbs[c]) for c in self.lists]
        self.bps, self.post_doc = bps, arrays["post_doc"]
        self.dots = [orc.summary_distances(desc, c, self.qc, self.qv) if n else np.zeros(0, np.float32) for c, n in zip(self.lists, self.nb)]
        self._score = {}

    def score(self, doc):
        s = self._score.get(doc)
        if s is None:
            s = self._score[doc] = float(_f32(orc.score_doc(self.desc, int(doc), self.qc, self.qv)))
        return s

    def postings(self, li, b):
        g = self.b0[li] + b
        return [int(d) for d in self.post_doc[self.bps[g]: self.bps[g + 1]]]


def schedule(case, desc, run, qname, cfg, reading=None):
    """One query of a forced run restated. cfg: the hook's words (block, max_cand, first_reach, dots_cap, qg, items_init,
    items_max). reading: None, or one of READINGS - a WRONG reading of the protocol, for test_coop_cases_cpu.py.
    Returns dict(scores, ids: the rows in front of a kNN refinement; rounds: [dict(kind, accepted, l, pos, end, n_pos, nc,
    thr0)]; spec: (lo, hi) of work counter [7] in front of a kNN refinement; live: per wide round the positions' liveness)."""
    a = orc.desc_arrays(desc)
    W = _Lists(case, desc, a, qname, min(run.cut, len(case.queries[qname][0])))
    k, hf = run.k, _f32(run.hf)
    NT, max_cand, reach = cfg["block"], cfg["max_cand"], cfg["first_reach"]
    heap = _Heap(k)
    rounds, lives = [], []
    spec_lo = spec_hi = 0
    nl = len(W.lists)
    sorted0 = bool(run.first_sorted) and nl > 0 and W.nb[0] > 1
    order0 = np.lexsort((np.arange(W.nb[0]), -W.dots[0].astype(np.float64))) if sorted0 else None   # dot descending, block ascending

    def block_at(li, i):
        if sorted0 and (li == 0 or reading == "order_every_list"):
            j = int(order0[i]) if i < len(order0) else i
            return j if j < W.nb[li] else i
        return i

    def cut_of(thr):
        return _f32(hf * _f32(thr))

    def seq_block(li, b, decided_live):
        """The sequential rule on one block: live at its start (or not full), then every posting in order. Returns
        (postings scored by the lower bound, postings)."""
        posts = W.postings(li, b)
        live = decided_live or not heap.full or not (W.dots[li][b] < cut_of(heap.thr))
        if live:
            for d in posts:
                s = W.score(d)
                if heap.contains(d):
                    continue
                if not heap.full or s > heap.thr:
                    heap.insert(s, d)
        return (len(posts) if (live or hf < 0) else 0), len(posts)

    def wide(l, pos, l1, limit):
        """wide_round: returns (accepted, l_end, pos_end)."""
        nonlocal spec_lo, spec_hi
        n_pos = sum(W.nb[li] - (pos if li == l else 0) for li in range(l, l1))
        n_pos = min(n_pos, limit)
        thr0 = heap.thr
        rec = dict(kind="wide", accepted=False, l=l, pos=pos, end=(l, pos), n_pos=n_pos, nc=None, thr0=thr0)
        rounds.append(rec)
        if n_pos == 0:
            lives.append([])
            return False, l, pos
        P, base, end = [], 0, (l, pos)
        for li in range(l, l1):
            if base >= n_pos:
                break
            first = pos if li == l else 0
            nb = W.nb[li] if W.nb[li] - first <= n_pos - base else first + (n_pos - base)
            P += [(li, block_at(li, i)) for i in range(first, nb)]
            base += nb - first
            end = (li + 1, 0) if nb == W.nb[li] else (li, nb)
        cut0 = cut_of(thr0) if hf >= 0 else _f32(-np.inf)
        cands, nc, live = [], 0, []
        for rp, (li, b) in enumerate(P):
            posts = W.postings(li, b)
            ok = (not (W.dots[li][b] < cut0)) and len(posts) > 0
            live.append(len(posts) if ok else 0)
            if not ok:
                continue
            spec_lo, spec_hi = spec_lo + len(posts), spec_hi + len(posts)
            for j, d in enumerate(posts):
                s = W.score(d)
                if s > thr0:
                    if j > KEY_MAX:
                        nc += 0x40000000
                    else:
                        nc += 1
                        cands.append(((rp << 16) | j, s, d, W.dots[li][b], rp))
        lives.append(live)
        rec["nc"] = nc
        if nc >= max_cand if reading == "overflow_ge" else nc > max_cand:
            return (False,) + (end if reading == "resume_at_end" else (l, pos))
        cands.sort()
        decided = None
        for c, (_, s, d, dot, rp) in enumerate(cands):
            if reading == "decided_per_window" and c % WINDOW == 0:
                decided = None
            if not s > heap.thr:
                continue
            if not (rp == decided or not (dot < cut_of(heap.thr))):
                continue
            if reading != "no_heap_contains" and heap.contains(d):
                continue
            heap.insert(s, d)
            decided = rp
        rec["accepted"], rec["end"] = True, end
        return True, end[0], end[1]

    wide_off = False
    budget = cfg["items_init"]
    l0 = 0
    while l0 < nl:
        l1, o = l0, 0
        while l1 < nl and (l1 == l0 or (o + W.nb[l1] <= cfg["dots_cap"] and l1 - l0 < cfg["qg"])):
            o += W.nb[l1]
            l1 += 1
        group_done, resume_pos, l = False, 0, l0
        while l < l1 and not group_done:
            nb = W.nb[l]
            pos, resume_pos = resume_pos, 0
            while pos < nb:
                if heap.full and not wide_off:
                    wl, wpos, limit, ok = l, pos, (0xffffffff if reading == "first_unbounded" else reach), True
                    while ok and wl < l1:
                        ok, wl, wpos = wide(wl, wpos, l1, limit)
                        limit = 0xffffffff
                    if ok:
                        group_done = True
                        break
                    wide_off = True
                    if wl != l:
                        resume_pos, l = wpos, wl - 1
                        break
                    pos = wpos
                    if pos >= nb:
                        break
                if not heap.full:
                    # a local round that starts with the heap not full: every block live, the first NT of them, a prefix by
                    # the item budget (always the first block)
                    sizes = [len(W.postings(l, block_at(l, i))) for i in range(pos, min(nb, pos + NT))]
                    B = min(max(budget, sizes[0]), max(cfg["items_max"], sizes[0]))
                    n, tot = 0, 0
                    while n < len(sizes) and tot + sizes[n] <= B:
                        tot += sizes[n]
                        n += 1
                    rounds.append(dict(kind="local", accepted=True, l=l, pos=pos, end=(l, pos + n), n_pos=n, nc=None, thr0=None))
                    for i in range(pos, pos + n):
                        seq_block(l, block_at(l, i), False)
                    spec_lo, spec_hi = spec_lo + tot, spec_hi + tot
                    pos += n
                    budget = min(budget * 2, cfg["items_max"])
                else:
                    # local rounds with a full heap (after a fallback): block by block, the sequential rule
                    lo, hi = seq_block(l, block_at(l, pos), False)
                    spec_lo, spec_hi = spec_lo + lo, spec_hi + hi
                    if not rounds or rounds[-1]["kind"] != "local_after_fallback" or rounds[-1]["end"] != (l, pos):
                        rounds.append(dict(kind="local_after_fallback", accepted=True, l=l, pos=pos, end=(l, pos), n_pos=0, nc=None, thr0=None))
                    rounds[-1]["end"], rounds[-1]["n_pos"] = (l, pos + 1), rounds[-1]["n_pos"] + 1
                    pos += 1
            l += 1
        l0 = l1
    n = len(heap.e)
    scores = np.zeros(k, np.float32)
    ids = np.zeros(k, np.uint64)
    scores[:n] = [s for s, _ in heap.e]
    ids[:n] = [d for _, d in heap.e]
    return dict(scores=scores, ids=ids, n=n, rounds=rounds, spec=(spec_lo, spec_hi), live=lives)


def cfg_of(h):
    return dict(block=h["block"], max_cand=h["max_cand"], first_reach=h["first_reach"], dots_cap=h["dots_cap"], qg=h["qg"],
                items_init=h["items_init"], items_max=h["items_max"])


# ---------------------------------------------------------------------------------------------------------------------
# units: blocks of one posting
# ---------------------------------------------------------------------------------------------------------------------
def _hits(i):
    return (65 + (i * 37) % 180) / 64.0


def _g0_tail(i):      # 3 hits among the first 30, then every other one
    hit = (i % 10 == 0) if i < 30 else (i % 2 == 0)
    return (70 + i % 50) / 64.0 if hit else (10 + i % 40) / 64.0


ONES = [1.0] * 64
U_LISTS = {
    "g0": ONES + [_g0_tail(i) for i in range(100)],
    "g1": [(70 + i % 60) / 64.0 if i % 4 == 0 else (8 + i % 50) / 64.0 for i in range(80)],
    "h0": ONES + [_hits(i) for i in range(200)] + [(5 + i % 55) / 64.0 for i in range(100)],
    "rnd": None,                                                                # 700 random values
    "c1": [(224 + i // 2) / 64.0 for i in range(60)],                           # 3.5 rising to 3.95
    "s0": [(128 + i) / 64.0 for i in range(64)] + [(10 + i) / 64.0 for i in range(20)],
    "mt": ONES + [(80 + i) / 64.0 for i in range(10)] + [(1 + i % 4) / 64.0 for i in range(256)],
    "tiny": [1.5],
}
U_LISTS.update({"n%d" % i: None for i in range(9)})                             # 70 random values each
U_ID = {n: i for i, n in enumerate(list(U_LISTS) + ["da", "db"])}
U_HOLE = 19                                                                     # a component no document has
U_DA_X, U_DB_X, U_DB_ONES, U_DB_NEW = 100, 50, 30, 20
U_QUERIES = {"geo": ("g0", "g1"), "one_list": ("g0",), "hits": ("h0", "rnd"), "two": ("s0", "c1"), "dup": ("da", "db"),
             "nine": tuple("n%d" % i for i in range(9)), "chunky": ("mt", "g1"), "kq": ("rnd", "g1"), "tiny": ("tiny",), "q1": ("h0",)}
U_POOL = ("hits", "empty", "tiny", "geo", "q255", "q1", "two")      # 7 queries: coprime to a grid of 512 workgroups
U_CYCLE = 1050
U_KNN = SC.U_KNN
MAX_GRID = 512              # workgroups of a cooperative launch at most (the open-round bitmap of its board has 512 bits)
SEQ_WRAP = 1024             # rounds of a workgroup after which its 10-bit round number comes round again
WRAP_CYCLE = 52000          # queries of the wrap run: `nine` and `geo` in turn, 18 + 4 rounds a pair
G0_REST = 100 + 80          # positions of `geo` behind its first local round of 64


def _units_runs(form):
    F = lambda n: dict(SGPU_COOP_FIRST_REACH=str(n))   # noqa: E731
    CH = lambda n: dict(SGPU_COOP_FIRST_REACH="131", SGPU_COOP_CHUNK=str(n), SGPU_COOP_CHUNK_MIN=str(n))   # noqa: E731
    runs = [
        # a. round geometry
        Run("reach_exact", "a: first round of exactly first_reach positions, ending at the group's end", ("geo",), 10, 2, 0.0, env=F(G0_REST)),
        Run("reach_minus1", "a: first_reach - 1: a second round of one position, the first ends inside a list", ("geo",), 10, 2, 0.0, env=F(G0_REST - 1)),
        Run("reach_plus1", "a: first_reach + 1 > what is left", ("geo",), 10, 2, 0.0, env=F(G0_REST + 1)),
        Run("reach_fewer", "a: fewer positions left than first_reach", ("geo",), 10, 2, 0.8, env=F(400)),
        Run("end_at_list_end", "a: the first round ends exactly at a list's end; a group of two lists", ("geo",), 10, 2, 0.0, env=F(100)),
        Run("end_inside", "a: the first round ends inside list 0", ("geo", "hits"), 10, 2, 0.8, env=F(50)),
        Run("one_list", "a: a group of one list", ("one_list",), 10, 1, 0.0, env=F(30)),
        Run("groups_4_4_1", "a: SGPU_LIST_GROUP=4 at query_cut 9", ("nine",), 10, 9, 0.8, env=dict(F(100), SGPU_LIST_GROUP="4")),
        Run("sorted_mid", "a: first_sorted, the round starts mid list 0 (order[] on list 0 only)", ("geo", "hits", "two"), 10, 2, 0.8, first_sorted=True, env=F(50)),
        Run("n_pos_0", "a: a second round with n_pos == 0 left (an empty list ends the group)", ("hole",), 10, 2, 0.0, env=F(400)),
        # b. candidate limit (the first round of `hits` under first_reach 40 has nc = 40)
        Run("cand_minus1", "b: nc = max_cand - 1", ("hits",), 10, 2, 0.0, env=dict(F(40), SGPU_COOP_MAX_CAND="41")),
        Run("cand_equal", "b: nc = max_cand: accepted", ("hits",), 10, 2, 0.0, env=dict(F(40), SGPU_COOP_MAX_CAND="40")),
        Run("cand_plus1", "b: nc = max_cand + 1 in the FIRST round: fallback in the same list", ("hits",), 10, 2, 0.0, env=dict(F(40), SGPU_COOP_MAX_CAND="39")),
        Run("cand_1", "b: SGPU_COOP_MAX_CAND=1", ("geo", "hits"), 10, 2, 0.0, env=dict(F(50), SGPU_COOP_MAX_CAND="1")),
        Run("cand_default", "b: the default limit (NT or what the union region holds): overflow at 512 threads, 12 windows at 1024", ("hits",), 10, 2, 0.0, env=F(2000)),
        Run("second_list_start", "b: overflow in the SECOND round, begun at the start of a later list (wl != l); list 0 sorted once", ("two",), 10, 2, 0.0,
            first_sorted=True, env=dict(F(20), SGPU_COOP_MAX_CAND="50")),
        Run("second_inside", "b: overflow in the SECOND round, begun inside a later list (resume_pos != 0)", ("two",), 10, 2, 0.0,
            first_sorted=True, env=dict(F(30), SGPU_COOP_MAX_CAND="45")),
        Run("second_same_list", "b: overflow in the second round in the group's last list, begun in the list of the first (wl == l)", ("one_list",), 10, 1, 0.0,
            env=dict(F(30), SGPU_COOP_MAX_CAND="5")),
        # d. replay
    ]
    runs += [Run("nc%d" % n, "d: nc = %d" % n, ("hits",), 10, 2, 0.0, env=F(n)) for n in (63, 64, 65, 129)]
    runs += [Run("factor%g" % hf, "d: heap_factor %g" % hf, ("hits", "geo", "dup", "neg"), 10, 2, hf, first_sorted=i % 2 == 1, env=F(100)) for i, hf in enumerate(FACTORS)]
    runs += [Run("dup", "d: a document in two lists of one wide round, and one already in the heap from the local round", ("dup",), 10, 2, 0.0, env=F(400))]
    runs += [Run("k%d" % k, "d: k = %d" % k, ("kq", "hits"), k, 2, 0.9, init=max(64, k), env=F(100)) for k in KS]
    runs += [Run("k%d" % K_PLAIN, "d: k = 257 takes the plain variant", ("kq",), K_PLAIN, 2, 0.9, init=300, env=F(100))]
    # e. chunks (first round of 131 positions, a prime: no multiple of any of these chunk sizes but 1)
    runs += [Run("chunk%d" % n, "e: SGPU_COOP_CHUNK %d (= CHUNK_MIN), n_pos no multiple of it; chunks of %s items" % (n, n if n < 6 else "many"),
                 ("hits",), 10, 2, 0.0, env=CH(n)) for n in (1, 3, 4, 5, 64, 1023, 1024)]
    runs += [Run("chunk_all_fail", "e: chunks whose blocks all fail the cut", ("chunky",), 10, 2, 1.0, env=dict(SGPU_COOP_FIRST_REACH="400", SGPU_COOP_CHUNK="64", SGPU_COOP_CHUNK_MIN="64")),
             Run("filtered", "e: a filtered run: whole blocks empty (cnt == 0)", ("geo", "hits", "chunky", "empty"), 10, 2, 0.0, filtered=True, env=F(100))]
    # g. helpers: launches of 1, 2 and 7 queries of 1 and 255 components in turn, under each lookup layout of the form
    layouts = {"u16_f16": (("dense", {}), ("packed", dict(SGPU_NO_DENSE="1"))),
               "u32_u8": (("packed", {}), ("split", dict(SGPU_FORCE_SPLIT="1"))),
               "u32_f16": (("packed", {}), ("split", dict(SGPU_FORCE_SPLIT="1")), ("hashed", dict(SGPU_FORCE_HASH="1")))}[form]
    for lname, lenv in layouts:
        for nq in (1, 2, 7):
            for mode in ("force", "auto"):
                runs.append(Run("helpers%d_%s_%s" % (nq, lname, mode), "g: %d queries of 1 / 255 components, %s lookup, %s" % (nq, lname, mode),
                                ("q1", "q255"), 10, 2, 0.8, mode=mode, cycle=nq, env=dict(F(100), **lenv)))
    # h. next query and board; j. kNN refinement
    runs += [Run("next_query", "h: seven queries in turn, more queries than workgroups", U_POOL, 10, 2, 0.8, cycle=U_CYCLE, env=F(100)),
             Run("wrap", "i: more than 1024 wide rounds of one workgroup in one launch (the 10-bit round number wraps)", ("nine", "geo"), 10, 9, 0.0,
                 cycle=WRAP_CYCLE, env=dict(SGPU_COOP_FIRST_REACH="1", SGPU_LIST_GROUP="1")),
             Run("knn1", "j: n_knn 1 behind a wide round", ("hits", "geo", "dup"), 10, 2, 0.8, n_knn=1, env=F(100)),
             Run("knn5", "j: n_knn 5 behind a wide round", ("hits", "geo", "dup"), 10, 2, 0.8, n_knn=5, env=F(100))]
    return runs


def _units(form):
    rng = np.random.default_rng(4004)
    pairs = [(i, j) for i in range(*SC.U_SIG) for j in range(i + 1, SC.U_SIG[1])]
    docs = []

    def add(heads, vals):
        s = pairs[len(docs) % len(pairs)]
        docs.append((np.array(list(heads) + [s[0], s[1]], np.int64), np.array(list(vals) + [3.0, 3.0], np.float32)))
        return len(docs) - 1

    for name, vals in U_LISTS.items():
        if vals is None:
            vals = rng.integers(8, 251, 700 if name == "rnd" else 70) / 64.0
        for x in vals:
            add([U_ID[name]], [x])
    # da: 64 ones, then 100 documents X; db: 50 of X (the high ones), 30 of da's ones, 20 of its own - in ascending id
    for i in range(64 + U_DA_X):
        heads, vals = [U_ID["da"]], [1.0 if i < 64 else (66 + (i * 29) % 150) / 64.0]
        if i < U_DB_ONES or i >= 64 + U_DA_X - U_DB_X:
            heads, vals = heads + [U_ID["db"]], vals + [(40 + (i * 13) % 100) / 64.0]
        add(heads, vals)
    for i in range(U_DB_NEW):
        add([U_ID["db"]], [(30 + i) / 64.0])
    assert len(docs) <= len(pairs)
    queries = {n: SC._q(rng, [U_ID[x] for x in lists], 2.0 - 0.125 * np.arange(len(lists))) for n, lists in U_QUERIES.items()}
    queries["hole"] = SC._q(rng, [U_ID["g0"], U_HOLE], [2.0, 1.875])
    c, v = SC._q(rng, [U_ID["g1"], U_ID["mt"]], [2.0, 1.875])
    queries["neg"] = (c, -v)                                       # walks mt first (-1.875): the ones, then far better documents
    queries["q255"] = SC._q(rng, [U_ID["rnd"], U_ID["g1"]], [2.0, 1.875], 253)
    queries["empty"] = SC.EMPTY_Q
    return CoopCase("units", form, len(docs), docs, queries, _units_runs(form), SC.UNIT_BLOCKS, _check_units)


def wide_rounds(res):
    """Rounds a query's owner opens on its slot (each advances the workgroup's round number): its wide rounds with n_pos > 0."""
    return sum(1 for r in res["rounds"] if r["kind"] == "wide" and r["n_pos"] > 0)


def _first_wide(res):
    return next(r for r in res["rounds"] if r["kind"] == "wide")


def restate(case, ix, run, block, qname, reading=None, **chip):
    desc = SC.FilteredDesc(ix.desc, case.allowed()) if run.filtered else None
    r = schedule(case, desc.desc if desc else ix.desc, run, qname, cfg_of(hook(case, ix, run, block, **chip)), reading)
    r["_keep"] = desc
    return r


def _check_units(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda name: int(case.phys([U_ID[name]])[0])   # noqa: E731
    found = {}
    assert (np.diff(a["block_post_start"].astype(np.int64)) == 1).all()               # every block is one posting
    for name in list(U_LISTS) + ["da", "db"]:
        d = SC.list_docs(a, P(name))
        assert np.array_equal(d, np.sort(d)), name                                    # traversal = ascending document id
    assert len(SC.list_blocks(a, P("g0"))) == 164 and len(SC.list_blocks(a, P("g1"))) == 80 and len(SC.list_blocks(a, int(case.phys([U_HOLE])[0]))) == 0
    assert len(SC.list_blocks(a, P("db"))) == U_DB_X + U_DB_ONES + U_DB_NEW
    for q, lists in U_QUERIES.items():
        assert SC.walked(case, q, len(lists)) == [P(x) for x in lists], q
    R = case.runs
    for block in BLOCKS:
        rs = lambda rn, q: restate(case, ix, R[rn], block, q)   # noqa: E731
        kinds = lambda res: [(r["kind"], r["accepted"]) for r in res["rounds"]]   # noqa: E731
        # a. geometry: the first local round is the 64 ones of list 0; what is left of the group is G0_REST positions
        for rn, want in (("reach_exact", [(G0_REST, (2, 0))]), ("reach_minus1", [(G0_REST - 1, (1, 79)), (1, (2, 0))]),
                         ("reach_plus1", [(G0_REST, (2, 0))]), ("reach_fewer", [(G0_REST, (2, 0))]),
                         ("end_at_list_end", [(100, (1, 0)), (80, (2, 0))]), ("end_inside", [(50, (0, 114)), (130, (2, 0))])):
            res = rs(rn, "geo")
            assert res["rounds"][0] == dict(kind="local", accepted=True, l=0, pos=0, end=(0, 64), n_pos=64, nc=None, thr0=None), (rn, res["rounds"][0])
            assert [(r["n_pos"], r["end"]) for r in res["rounds"][1:]] == want and all(r["accepted"] for r in res["rounds"]), (rn, block, res["rounds"])
            assert (res["rounds"][1]["l"], res["rounds"][1]["pos"]) == (0, 64)
        res = rs("one_list", "one_list")
        assert [(r["n_pos"], r["end"]) for r in res["rounds"]] == [(64, (0, 64)), (30, (0, 94)), (70, (1, 0))]
        res = rs("groups_4_4_1", "nine")
        starts = [(r["l"], r["pos"]) for r in res["rounds"] if r["kind"] == "wide"]
        assert {(4, 0), (8, 0)} <= set(starts) and all(r["accepted"] for r in res["rounds"]), starts      # every group goes wide from its start
        assert hook(case, ix, R["groups_4_4_1"], block)["qg"] == 4
        res = rs("sorted_mid", "geo")
        w = _first_wide(res)
        assert (w["l"], w["pos"]) == (0, 64) and w["accepted"]
        res = rs("n_pos_0", "hole")
        assert [(r["kind"], r["n_pos"], r["accepted"]) for r in res["rounds"]] == [("local", 64, True), ("wide", 100, True), ("wide", 0, False)], res["rounds"]
        # b. the candidate limit, against the max_cand the hook reports
        for rn, d, ok in (("cand_minus1", -1, True), ("cand_equal", 0, True), ("cand_plus1", 1, False)):
            res, mc = rs(rn, "hits"), hook(case, ix, R[rn], block)["max_cand"]
            w = _first_wide(res)
            assert w["nc"] == mc + d == 40 and w["accepted"] == ok and (w["l"], w["pos"]) == (0, 64), (rn, block, w, mc)
            if not ok:
                assert res["rounds"][2]["kind"] == "local_after_fallback" and (res["rounds"][2]["l"], res["rounds"][2]["pos"]) == (0, 64)
                assert res["spec"][0] == res["spec"][1] == 64 + 40 + (300 + 700)          # the round's 40 are scored twice
        assert hook(case, ix, R["cand_1"], block)["max_cand"] == 1
        w = _first_wide(rs("cand_1", "hits"))
        assert w["nc"] == 50 and not w["accepted"]
        mc = hook(case, ix, R["cand_default"], block)["max_cand"]
        w = _first_wide(rs("cand_default", "hits"))
        # (711 candidates: more than a 512-thread workgroup can rank - fallback; a 1024-thread one replays them in 12 windows)
        assert mc <= block and w["nc"] > 512 and w["accepted"] == (w["nc"] <= mc) == (block == 1024), (block, mc, w)
        found["max_cand_default_%d" % block] = (mc, w["nc"])
        res = rs("second_list_start", "two")
        assert [(r["kind"], r["accepted"], r["l"], r["pos"]) for r in res["rounds"]] == [
            ("local", True, 0, 0), ("wide", True, 0, 64), ("wide", False, 1, 0), ("local_after_fallback", True, 1, 0)], res["rounds"]
        res = rs("second_inside", "two")
        assert [(r["kind"], r["accepted"], r["l"], r["pos"]) for r in res["rounds"]] == [
            ("local", True, 0, 0), ("wide", True, 0, 64), ("wide", False, 1, 10), ("local_after_fallback", True, 1, 10)], res["rounds"]
        res = rs("second_same_list", "one_list")
        assert [(r["kind"], r["accepted"], r["l"], r["pos"]) for r in res["rounds"]] == [
            ("local", True, 0, 0), ("wide", True, 0, 64), ("wide", False, 0, 94), ("local_after_fallback", True, 0, 94)], res["rounds"]
        # d. replay windows, documents met twice, heap variants
        for n in (63, 64, 65, 129):
            w = _first_wide(rs("nc%d" % n, "hits"))
            assert w["nc"] == n and w["accepted"], (n, w)
        res = rs("dup", "dup")
        w = _first_wide(res)
        assert w["accepted"] and w["n_pos"] == U_DA_X + U_DB_X + U_DB_ONES + U_DB_NEW
        da, db = SC.list_docs(a, P("da")), SC.list_docs(a, P("db"))
        top = set(int(x) for x in res["ids"][: res["n"]])
        assert len(top & set(da[64:].tolist()) & set(db.tolist())) >= 3, top      # rows hold documents the round met twice
        assert len(np.intersect1d(da[:64], db)) == U_DB_ONES                      # and the round meets documents of the local round again
        for k in KS:
            for q in ("kq", "hits"):
                res = rs("k%d" % k, q)
                ws = [r for r in res["rounds"] if r["kind"] == "wide"]
                assert res["n"] == k and ws and all(r["accepted"] for r in ws) and sum(r["nc"] for r in ws) >= 1, (k, q, res["rounds"])
        assert hook(case, ix, R["k%d" % K_PLAIN], block)["coop"] == 0
        for hf in FACTORS:
            res = rs("factor%g" % hf, "neg")
            # (under first_sorted the best blocks come first: the rounds then return no candidate)
            assert (res["scores"][: res["n"]] < 0).all() and any(r["kind"] == "wide" and r["accepted"] and (r["nc"] or R["factor%g" % hf].first_sorted)
                                                                 for r in res["rounds"]), (hf, res["rounds"])
        # e. chunks
        for n in (1, 3, 4, 5, 64, 1023, 1024):
            h = hook(case, ix, R["chunk%d" % n], block)
            want = min(n, 1023, block)
            assert h["chunk"] == h["chunk_min"] == want, (n, block, h["chunk"], h["chunk_min"])
            res = rs("chunk%d" % n, "hits")
            w = _first_wide(res)
            assert w["n_pos"] == 131 and w["accepted"] and (131 % want != 0 or want == 1)
            if n <= 5:
                assert all(x == 1 for x in res["live"][0])                        # heap_factor 0: every chunk holds exactly `chunk` items
        res = rs("chunk_all_fail", "chunky")
        live = res["live"][0]
        dead = [c for c in range(0, len(live), 64) if not any(live[c: c + 64])]
        assert len(dead) >= 2 and any(live), dead
        found["chunks_all_fail_%d" % block] = dead
        fd = SC.FilteredDesc(ix.desc, case.allowed())
        cnt = np.diff(fd.bps.astype(np.int64))
        assert (cnt == 0).sum() >= 100 and (cnt == 1).sum() >= 100
        res = rs("filtered", "hits")
        assert any(r["kind"] == "wide" for r in res["rounds"])
        # g. helpers: the queries alternate across the dense table's scaled / plain boundary (63 | 64 components)
        assert len(case.queries["q1"][0]) == 1 and len(case.queries["q255"][0]) == 255
        # i. the wrap: with first_reach 1 and one list per group every group but a query's first takes two wide rounds (one
        # position, then the rest). Whatever the workgroups' shares of the queries, the rounds of the launch exceed 1024 x
        # the largest grid there is: some workgroup opens more than 1024
        r = R["wrap"]
        per = [wide_rounds(rs("wrap", q)) for q in r.queries]
        assert per == [18, 4], per
        assert all(x["accepted"] for q in r.queries for x in rs("wrap", q)["rounds"])
        total = sum(per[i % len(per)] for i in range(r.cycle))
        assert total > SEQ_WRAP * MAX_GRID, total
        found["wrap_rounds"] = total
        # h. more queries than a cooperative launch has workgroups (512 at most), 7 coprime to it
        r = R["next_query"]
        assert len(r.queries) == 7 and r.cycle % 7 == 0 and r.cycle > 512 and np.gcd(512, 7) == 1
    return found


# ---------------------------------------------------------------------------------------------------------------------
# blocks: one block per list
# ---------------------------------------------------------------------------------------------------------------------
B_LENGTHS = (1, 8, 127, 128, 129, 256, 257, 600)
B_FIRST, B_LEN, B_RISE, B_BIG, B_A, B_B = 0, 1, 2, 3, 4, 5
B_N = {B_FIRST: 100, B_LEN: 320, B_RISE: 200, B_BIG: 3000}
B_A_DOCS, B_B_FROM, B_B_DOCS = 100, 70, 100
B_QUERIES = {"lens": (B_FIRST, B_LEN), "straddle": (B_FIRST, B_RISE), "big": (B_FIRST, B_BIG), "dup": (B_FIRST, B_A, B_B),
             "all": (B_FIRST, B_LEN, B_RISE, B_A, B_B)}


def _bdoc(rng, far_ok, heads, head_vals, n, far):
    """One document of n components: its list components, then body components with SMALL values (the list component
    carries the block's summary)."""
    nb = n - len(heads)
    assert nb >= 0
    body = rng.choice(np.arange(*SC.BODY), nb, replace=False)
    if far and far_ok and nb >= 1:
        body[-1] = int(rng.integers(*SC.FAR))
    c = np.concatenate([np.asarray(heads, np.int64), np.sort(body)])
    v = np.concatenate([np.asarray(head_vals, np.float32), (rng.integers(1, 9, nb) / 64.0).astype(np.float32)])
    order = np.argsort(c, kind="stable")
    return c[order], v[order]


def _blocks(form):
    rng = np.random.default_rng(5005)
    far = SC.FORMS[form][1] == 2
    docs = []
    for i in range(B_N[B_FIRST]):
        docs.append(_bdoc(rng, far, [B_FIRST], [(32 + i % 26) / 64.0], int(rng.integers(3, 11)), i % 3 == 0))          # 0.5 .. 0.89
    for i in range(B_N[B_LEN]):
        n = B_LENGTHS[(i // 2) % len(B_LENGTHS)] if i % 2 == 0 else int(rng.integers(2, 300))
        docs.append(_bdoc(rng, far, [B_LEN], [int(rng.integers(8, 251)) / 64.0], n, i % 4 >= 2))
    for i in range(B_N[B_RISE]):
        docs.append(_bdoc(rng, far, [B_RISE], [(56 + i) / 64.0], int(rng.integers(2, 7)), False))                         # 0.875 rising to 3.98
    for i in range(B_N[B_BIG]):
        v = (200 + i % 50) / 64.0 if i % 30 == 7 else (4 + i % 40) / 64.0                                                 # 100 high ones
        docs.append(_bdoc(rng, far, [B_BIG], [v], int(rng.integers(2, 5)), False))
    for i in range(B_B_FROM + B_B_DOCS):
        heads = ([B_A] if i < B_A_DOCS else []) + ([B_B] if i >= B_B_FROM else [])
        docs.append(_bdoc(rng, far, heads, (rng.integers(60, 250, len(heads)) / 64.0), int(rng.integers(3, 30)), i % 5 == 0))
    queries = {n: SC._q(rng, lists, 2.0 - 0.125 * np.arange(len(lists))) for n, lists in B_QUERIES.items()}   # (list components only)
    c, v = SC._q(rng, (B_FIRST, B_LEN, B_RISE), (2.0, 1.875, 1.75))
    queries["neg"] = (c, -v)
    queries["empty"] = SC.EMPTY_Q
    F = dict(SGPU_COOP_FIRST_REACH="100")
    runs = [Run("lengths", "f: documents of 1 ... 600 components (the eb loop), raw DotVByte records among them", ("lens", "all", "empty"), 10, 5, 0.0, env=F),
            Run("lengths_k129", "f: the same under k = 129", ("lens", "all"), 129, 5, 0.9, env=F)]
    runs += [Run("straddle%g" % hf, "d: a block whose surviving items straddle 64-candidate windows (decided carries over), heap_factor %g" % hf,
                 ("straddle", "all", "neg"), 10, 5, hf, env=F) for hf in FACTORS]
    runs += [Run("big_chunk", "e: a chunk of one position holding 3000 items", ("big",), 10, 2, 0.0, env=dict(F, SGPU_COOP_CHUNK="1", SGPU_COOP_CHUNK_MIN="1")),
             Run("dup", "d: the same document in two lists of one wide round", ("dup",), 10, 3, 0.0, env=F),
             Run("sorted", "a: first_sorted with one block per list", ("all", "dup"), 10, 5, 0.8, first_sorted=True, env=F),
             Run("filtered", "e: a filtered run", ("all", "lens", "big"), 10, 5, 0.0, filtered=True, env=F),
             Run("auto", "g: auto mode, rows only", ("all", "lens", "big", "dup"), 10, 5, 0.8, mode="auto", env=F)]
    return CoopCase("blocks", form, len(docs), docs, queries, runs, SC.ONE_BLOCK, _check_blocks)


def _check_blocks(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda lst: int(case.phys([lst])[0])   # noqa: E731
    found = {}
    for lst, size in B_N.items():
        assert SC.list_blocks(a, P(lst)).tolist() == [size], (lst, SC.list_blocks(a, P(lst)))
    assert SC.list_blocks(a, P(B_A)).tolist() == [B_A_DOCS] and SC.list_blocks(a, P(B_B)).tolist() == [B_B_DOCS]
    for q, lists in B_QUERIES.items():
        assert SC.walked(case, q, len(lists)) == [P(i) for i in lists], q
    lens = np.diff(a["fwd_offsets"].astype(np.int64))
    got = lens[SC.list_docs(a, P(B_LEN))]
    assert set(B_LENGTHS) <= set(got.tolist()) and (got > 128).sum() >= 40 and (got > 256).sum() >= 20
    if case.value_type == 2:
        raw = SC.raw_documents(a)
        assert raw[SC.list_docs(a, P(B_LEN))].sum() >= 20 and (~raw).sum() >= 20
        found["raw_documents"] = int(raw.sum())
    R = case.runs
    for block in BLOCKS:
        rs = lambda rn, q: restate(case, ix, R[rn], block, q)   # noqa: E731
        # the first local round is list 0's one block; the wide round covers the other lists, and is accepted
        res = rs("lengths", "lens")
        assert [(r["kind"], r["accepted"], r["l"], r["pos"], r["n_pos"]) for r in res["rounds"]] == [("local", True, 0, 0, 1), ("wide", True, 1, 0, 1)], res["rounds"]
        assert res["rounds"][1]["nc"] >= 65 and res["spec"] == (100 + 320, 100 + 320)
        # the straddle: one position, hundreds of candidates, the block dead against the threshold at the later windows' starts
        res = rs("straddle1.3", "straddle")
        w = _first_wide(res)
        assert w["accepted"] and w["n_pos"] == 1 and w["nc"] > 2 * WINDOW, w
        rise = SC.list_docs(a, P(B_RISE))
        assert set(int(x) for x in res["ids"][: res["n"]]) == set(rise[-10:].tolist())          # the block's last items are the result
        found["straddle_nc_%d" % block] = w["nc"]
        res = rs("big_chunk", "big")
        w = _first_wide(res)
        assert w["accepted"] and res["live"][0] == [B_N[B_BIG]] and 1 <= w["nc"] <= 120, w
        res = rs("dup", "dup")
        w = _first_wide(res)
        da, db = SC.list_docs(a, P(B_A)), SC.list_docs(a, P(B_B))
        assert w["accepted"] and w["n_pos"] == 2 and len(np.intersect1d(da, db)) == B_A_DOCS - B_B_FROM
        assert len(set(int(x) for x in res["ids"][: res["n"]]) & set(np.intersect1d(da, db).tolist())) >= 3
        for hf in FACTORS:
            res = rs("straddle%g" % hf, "neg")
            assert (res["scores"][: res["n"]] < 0).all() and any(r["kind"] == "wide" for r in res["rounds"])
    return found


# ---------------------------------------------------------------------------------------------------------------------
# big: one block of exactly 65 536 postings (the last one still has a key) and one of 65 537 (it has none)
# ---------------------------------------------------------------------------------------------------------------------
G_FIRST, G_KEY, G_NOKEY = 0, 1, 2
G_N = {G_FIRST: 100, G_KEY: KEY_MAX + 1, G_NOKEY: KEY_MAX + 2}
G_QUERIES = {"keyable": (G_FIRST, G_KEY), "unkeyable": (G_FIRST, G_NOKEY)}
G_CFG = dict(SC.ONE_BLOCK, n_postings=70000)


def _big(form):
    rng = np.random.default_rng(6006)
    docs = []
    for lst, n in G_N.items():
        i = np.arange(n)
        if lst == G_FIRST:
            v = (32 + i % 26) / 64.0                                              # 0.5 .. 0.89
        else:                                                                     # low, a high one every 1000, the LAST one the best
            v = np.where(i % 1000 == 500, (200 + i // 1000 % 50) / 64.0, (4 + i % 40) / 64.0)
            v[-1] = 255 / 64.0
        body = rng.integers(SC.BODY[0], SC.BODY[1], n)
        bv = rng.integers(1, 9, n) / 64.0
        for j in range(n):                                                        # two components: the list's and a small one
            docs.append((np.array([lst, body[j]], np.int64), np.array([v[j], bv[j]], np.float32)))
    queries = {n: SC._q(rng, lists, 2.0 - 0.125 * np.arange(len(lists))) for n, lists in G_QUERIES.items()}
    F = dict(SGPU_COOP_FIRST_REACH="100")
    runs = [Run("keyable", "c: one block of exactly 65 536 postings: every posting has a key, the last one is a candidate", ("keyable",), 10, 2, 0.0, env=F),
            Run("unkeyable", "c: one block of 65 537 postings: the last one has no key - fallback, rows still the oracle's", ("unkeyable",), 10, 2, 0.0, env=F),
            Run("both", "c: the two in one launch", ("keyable", "unkeyable"), 10, 2, 0.0, env=F)]
    return CoopCase("big", form, len(docs), docs, queries, runs, G_CFG, _check_big)


def _check_big(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda lst: int(case.phys([lst])[0])   # noqa: E731
    for lst, size in G_N.items():
        assert SC.list_blocks(a, P(lst)).tolist() == [size], (lst, SC.list_blocks(a, P(lst)))
    assert G_N[G_KEY] == 65536 and G_N[G_NOKEY] == 65537
    for q, lists in G_QUERIES.items():
        assert SC.walked(case, q, len(lists)) == [P(i) for i in lists], q
    found = {}
    for block in BLOCKS:
        mc = hook(case, ix, case.runs["keyable"], block)["max_cand"]
        res = restate(case, ix, case.runs["keyable"], block, "keyable")
        w = _first_wide(res)
        last = int(SC.list_docs(a, P(G_KEY))[-1])
        assert w["accepted"] and w["n_pos"] == 1 and res["live"][0] == [65536] and 1 <= w["nc"] <= mc, (block, w, mc)
        assert int(res["ids"][0]) == last                          # the posting with key 0xffff is the best row
        assert res["spec"] == (100 + 65536,) * 2
        res = restate(case, ix, case.runs["unkeyable"], block, "unkeyable")
        w = _first_wide(res)
        last = int(SC.list_docs(a, P(G_NOKEY))[-1])
        assert not w["accepted"] and w["n_pos"] == 1 and 0x40000000 <= w["nc"] < 0x40000000 + mc, (block, w, mc)   # ONE posting without a key, nothing else overflows
        assert [(r["kind"], r["l"], r["pos"]) for r in res["rounds"]] == [("local", 0, 0), ("wide", 1, 0), ("local_after_fallback", 1, 0)]
        assert int(res["ids"][0]) == last                          # ... and it is the best row: dropping it would show
        assert res["spec"] == (100 + 2 * 65537,) * 2               # the block is scored by the round and again by the local rounds
        found["nc_%d" % block] = w["nc"]
    return found


# ---------------------------------------------------------------------------------------------------------------------
KINDS = {"units": (_units, ("u16_f16", "u32_f16", "u32_u8")),
         "blocks": (_blocks, ("u16_u8", "u16_dvb")),
         "big": (_big, ("u16_f16",))}
CASE_NAMES = tuple("%s-%s" % (k, f) for k, (_, forms) in KINDS.items() for f in forms)
# wrong reading -> (case, run, query, what must differ: "rows" = the restated rows are no longer the oracle's, "rounds" = the
# round list or counter [7] is another one, so the device's counter tells the readings apart)
WRONG = {"overflow_ge": ("units-u16_f16", "cand_equal", "hits", "rounds"),
         "resume_at_end": ("units-u16_f16", "second_inside", "two", "rows"),
         "decided_per_window": ("blocks-u16_u8", "straddle1.3", "straddle", "rows"),
         "no_heap_contains": ("units-u16_f16", "dup", "dup", "rows"),
         "first_unbounded": ("units-u16_f16", "end_inside", "geo", "rounds"),
         "order_every_list": ("units-u16_f16", "sorted_mid", "geo", "rounds")}


@functools.lru_cache(maxsize=None)
def make(name):
    """The case `name` = "<kind>-<form>" (built once per process; its arrays are read-only)."""
    kind, form = name.split("-")
    return KINDS[kind][0](form)
