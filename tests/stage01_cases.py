"""Seeded inputs for the tests of stage 0 and stage 1 of the search kernel (seismic_amd/csrc/search_stage01.inc) at their
structural edges (test_stage01_cases_cpu.py, test_gpu_stage01_edges.py). TEST INFRASTRUCTURE, pure numpy apart from the
index build. Helpers of stream_cases.py, orc.py, model64.py and util.py are imported, not copied.

A case = a collection in one index form, named queries, DOTS (list, query) pairs observed through summary_distances (the
kernel's MODE_DOTS), RUNS (searches, each there for one edge) and a check() that asserts from the descriptor's arrays, a
numpy restatement of pack_row_mid (mids) and the project's CPU hooks alone that every edge is present.

Exact sizes (stream_cases.py): centroid_fraction 1.0 with two heavy signature components per document gives blocks of ONE
posting in ascending document id, summary_energy 1.0 keeps every component, n_postings exceeds every list. Block b of a
list is its b-th document and the summary row of (list c, component j) has one entry per document of c that holds j, so
a row's two halves (block ids below / from (nb + 1) / 2) are sized by choosing which documents carry j.

  rows       halves of 0, 1, 63, 64, 65, 127, 128, 129 entries, mid == 0, mid == len, absent rows first / last / inside a
             64-row block, a 64-row block empty in one half, lists of 300 and 301 blocks, signed weights of mixed magnitude
  chunks     one 64-row block with 1 ... 129 chunks in a half; chunks 63 and 64 of the same row
  pairs      queries of 1 ... 513 components on one list; searches of 4 x 32, 4 x 64 and 5 x 64 (list, component) pairs
  directory  u16: a displaced key, a key wrapped from the last bucket to bucket 0, an absent key whose home bucket is full;
             u32: lists of 0, 1, 2, 3 rows, targets below, between and above the rows
  groups     SGPU_LIST_GROUP 1 / 2 / 3, SGPU_DOTS_CAP at and one below the first two lists' blocks, an empty list inside a
             group, qg == query_cut at 9 and 5 (more streams than wavefronts)
  select     600 and 1100 equal weights, equal pairs across the cut, negative and zero weights, query_cut 0 ... nnz + 1
  lookup     a workgroup's next query under every lookup layout, dim % 4 and dim % 32 varied, component dim - 1
  sort       first_sorted over first lists of 2 ... 2049 blocks with equal and negative dots
"""
import functools

import numpy as np

import coop_cases as CC
import hash_cases as H
import model64 as M64
import orc
import stream_cases as SC
from seismic_amd import _native
from stream_cases import Run
from util import row_dir_bucket, row_dir_lookup, row_dir_table

BLOCKS = (512, 1024)                 # SGPU_BLOCK
SIG = (20, 100)                      # signature components (two per document, value 3.0)
CTL0 = 100                           # first component the cases hand out to shape rows
SIZES = (0, 1, 63, 64, 65, 127, 128, 129)
UNIT = dict(SC.UNIT_BLOCKS, n_postings=5000)
ONE = dict(SC.ONE_BLOCK)
ONE_FULL = dict(ONE, summary_energy=1.0)          # one block per list, every component in its summary
LOOKUP = {"packed": 0, "dense": 1, "split": 2, "hashed": 3}     # device_types.hpp: LK_*
_PAIRS = [(i, j) for i in range(*SIG) for j in range(i + 1, SIG[1])]
f32 = np.float32
U32_BASE = 65536                     # u32 forms: every component id lies above 2^16


class Case(SC.StreamCase):
    def __init__(self, kind, form, docs, queries, runs, cfg, check, dots=(), logical_dim=1000, dim=None, tag=""):
        self.kind, self.form = kind, form
        self.name = "-".join(x for x in (kind, form, tag) if x)
        self.cw, self.value_type = SC.FORMS[form]
        self.logical_dim = logical_dim
        self.dim = dim if dim is not None else (U32_BASE + 70 * logical_dim if self.cw == 4 else logical_dim)
        self.n_docs, self.cfg, self._check = len(docs), cfg, check
        self.off, self.comps, self.vals = orc.csr([(self.phys(c), v) for c, v in docs])
        self.queries = {n: (self.phys(c), np.asarray(v, f32)) for n, (c, v) in queries.items()}
        self.runs = {r.name: r for r in runs}
        self.dots = tuple(dots)          # (logical list, query name)
        for a in (self.off, self.comps, self.vals):
            a.setflags(write=False)

    def phys(self, c):
        """Logical ids -> the index's: u32 forms spread them 70 x above 2^16 (every id); the last logical id is dim - 1."""
        c = np.asarray(c, np.int64)
        if self.cw != 4:
            return c.astype(np.uint32)
        return np.where(c == self.logical_dim - 1, self.dim - 1, U32_BASE + c * 70).astype(np.uint32)

    def P(self, c):
        return int(self.phys([c])[0])


def srun(name, queries, k, cut, hf, expect=None, coop=False, **kw):
    r = Run(name, queries, k, cut, hf, **kw)
    r.expect, r.coop = dict(expect or {}), coop
    return r


def knob_env(case, run, block):
    """The environment a run is launched under: plain (streamed) unless the run asks for SGPU_COOP=force."""
    env = dict(SGPU_BLOCK=str(block), SGPU_COOP="force" if run.coop else "0")
    if SC.FORMS[case.form] == (4, 0) and "SGPU_FORCE_HASH" not in run.env:
        env["SGPU_NO_HASH"] = "1"      # (unforced runs keep the other layouts; the hashed lookup has test_gpu_hash_lookup.py)
    env.update(run.env)
    return env


def hook(case, ix, run, block, **over):
    """sgpu_debug_launch_config for a run under its knobs (no device)."""
    Q = case.batch(run)
    with CC.knobs(knob_env(case, run, block)):
        return _native.debug_launch_config(heap_factor=run.hf, **dict(SC.plan_facts(case, ix, run, Q), **over))


def _weights(rng, n, big=True):
    """Signed weights of mixed magnitude: +-2^12, +-1, +-2^-10, each times 1, 1.25, 1.5 or 1.75 (big=False: below 2)."""
    mag = rng.choice([4096.0, 1.0, 2.0 ** -10] if big else [1.0, 2.0 ** -10], n) * rng.choice([1.0, 1.25, 1.5, 1.75], n)
    return (mag * rng.choice([-1.0, 1.0], n)).astype(f32)


def _unit_doc(rng, n, lst, ctl, ctl_vals=None, lst_val=None):
    """Document n of a unit-block collection: its list component, its own signature pair (3.0, 3.0), the given others."""
    s = _PAIRS[n % len(_PAIRS)]
    ctl = np.asarray(ctl, np.int64)
    c = np.concatenate([[lst, s[0], s[1]], ctl])
    v = np.concatenate([[rng.integers(1, 33) / 64.0 if lst_val is None else lst_val, 3.0, 3.0],
                        rng.integers(1, 33, len(ctl)) / 64.0 if ctl_vals is None else ctl_vals])
    o = np.argsort(c, kind="stable")
    assert len(np.unique(c)) == len(c)
    return c[o], v[o].astype(f32)


def _sorted_q(c, v):
    o = np.argsort(np.asarray(c, np.int64), kind="stable")
    return np.asarray(c, np.int64)[o], np.asarray(v, f32)[o]


# ---------------------------------------------------------------------------------------------------------------------
# what the checks read, and the restatement of the kernel's walk
# ---------------------------------------------------------------------------------------------------------------------
def mids(a, split="up"):
    """pack_row_mid restated: per summary row, the entries whose block id is below (nb + 1) / 2 (split="down": the wrong
    reading nb / 2)."""
    lbs, lrs, rp = (a[n].astype(np.int64) for n in ("list_block_start", "list_row_start", "row_ptr"))
    nb = np.diff(lbs)
    half = (nb + 1) // 2 if split == "up" else nb // 2
    row_list = np.repeat(np.arange(len(nb)), np.diff(lrs))
    ent_row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    below = a["sum_bid"].astype(np.int64) < half[row_list][ent_row]
    return np.bincount(ent_row, below, len(rp) - 1).astype(np.int64)


def row_table(a, mid, c, comps):
    """build_row_table restated: (start, len, mid) of the row of (list c, component) for every query component; an
    absent row is (0, 0, 0)."""
    lrs, rp = a["list_row_start"].astype(np.int64), a["row_ptr"].astype(np.int64)
    rc = a["row_comp"][lrs[c]: lrs[c + 1]].astype(np.int64)
    comps = np.asarray(comps, np.int64)
    at = np.searchsorted(rc, comps)
    ok = (at < len(rc)) & (rc[np.minimum(at, max(len(rc) - 1, 0))] == comps) if len(rc) else np.zeros(len(comps), bool)
    r = lrs[c] + np.where(ok, at, 0)
    z = np.zeros(len(comps), np.int64)
    if not len(rc):
        return z, z.copy(), z.copy()
    return np.where(ok, rp[r], 0), np.where(ok, rp[r + 1] - rp[r], 0), np.where(ok, mid[r], 0)


def chunk_prefix(counts, carry=True):
    """The wave scan of rt_pre over blocks of 64 components (carry=False: the wrong reading without it)."""
    pre = np.zeros(len(counts) + 1, np.int64)
    run = 0
    for j0 in range(0, len(counts), 64):
        x = np.cumsum(counts[j0: j0 + 64])
        pre[j0 + 1: j0 + 1 + len(x)] = x + (run if carry else 0)
        run += int(x[-1]) if len(x) == 64 else 0
    return pre


def walk_dots(a, mid, c, comps, vals, round_up=True, owner="last", last64=False, carry=True, descending=False):
    """The kernel's walk on the descriptor: row table -> split -> chunk prefix -> owner search -> float32
    acc[bid] = acc[bid] + deq * w, stream by stream, block of 64 rows by block, chunk by chunk. The keyword arguments are
    the WRONG readings the cases must catch. Returns the block dots of list c (float32)."""
    lbs = a["list_block_start"].astype(np.int64)
    b0, nb = int(lbs[c]), int(lbs[c + 1] - lbs[c])
    acc = np.zeros(nb, f32)
    nnz = len(comps)
    if nb == 0 or nnz == 0:
        return acc
    start, ln, md = row_table(a, mid, c, comps)
    w = np.asarray(vals, f32)
    bid_all, code, quant, mn = a["sum_bid"], a["sum_code"], a["blk_quant"], a["blk_min"]
    ops = []                                                    # (first entry, entries, weight) in the order of execution
    for h in (0, 1):
        s_h, l_h = (start + md, ln - md) if h else (start, md)
        cpre = chunk_prefix((l_h + 63) >> 6 if round_up else l_h >> 6, carry)
        for jb in range(0, nnz, 64):
            nj = min(64, nnz - jb)
            lane = np.arange(64)
            c0 = cpre[jb + np.where(lane < nj, lane, nj)]
            t_begin, t_end = int(c0[0]), int(cpre[jb + nj])
            for x in range(t_begin, t_end):
                lo, hi = 0, 64
                for _ in range(6):
                    m = (lo + hi) >> 1
                    if c0[m] <= x:
                        lo = m
                    else:
                        hi = m
                if owner == "first":
                    lo = int(np.flatnonzero(c0 == c0[lo])[0])
                if lo >= nj:
                    continue                                      # (a lane past the block's rows: r = 0, no entries)
                u = x - int(c0[lo])
                n = 64 if last64 else max(0, min(64, int(l_h[jb + lo]) - u * 64))
                ops.append((int(s_h[jb + lo]) + u * 64, n, w[jb + lo]))
    for e0, n, wt in (reversed(ops) if descending else ops):
        e = np.arange(e0, min(e0 + n, len(bid_all)))
        b = bid_all[e].astype(np.int64)
        b = np.minimum(b, nb - 1)                                 # (only a wrong reading leaves the list's blocks)
        deq = (code[e].astype(f32) * quant[b0 + b]).astype(f32) + mn[b0 + b]
        acc[b] = acc[b] + (deq.astype(f32) * wt).astype(f32)
    return acc


def half_lens(a, mid, c, comps):
    _, ln, md = row_table(a, mid, c, comps)
    return md, ln - md


def plan_groups(nbs, dots_cap, qg, strict=False):
    """plan_list_group restated: the list groups of a walk over lists of nbs blocks (strict: `<` for `<=`)."""
    out, l = [], 0
    while l < len(nbs):
        o, l0 = 0, l
        while l < len(nbs) and (l == l0 or ((o + nbs[l] < dots_cap if strict else o + nbs[l] <= dots_cap) and l - l0 < qg)):
            o += nbs[l]
            l += 1
        out.append(list(range(l0, l)))
    return out


def walked(case, query, cut, ties="ascending"):
    """select_lists restated by the reference's rule: value descending (f32 total order), ties by ascending component
    (ties="descending": the wrong reading)."""
    c, v = case.queries[query]
    c = c.astype(np.int64)
    key = v.astype(np.float64)
    order = np.lexsort((c if ties == "ascending" else -c, -key))
    return [int(x) for x in c[order[: max(0, min(cut, len(c)))]]]


def _nb(a, c):
    return int(a["list_block_start"][c + 1] - a["list_block_start"][c])


def _unit_blocks(case, a, lists):
    """Every named list: blocks of one posting in ascending document id."""
    for lst in lists:
        c = case.P(lst)
        assert (SC.list_blocks(a, c) == 1).all(), lst
        d = SC.list_docs(a, c)
        assert np.array_equal(d, np.sort(d)), lst


def _order_sensitive(case, a, mid):
    """At least one accumulator of the case's dots differs in float32 between ascending and descending order."""
    n = 0
    for lst, q in case.dots:
        up = walk_dots(a, mid, case.P(lst), *case.queries[q])
        down = walk_dots(a, mid, case.P(lst), *case.queries[q], descending=True)
        n += int((up.view(np.uint32) != down.view(np.uint32)).sum())
    assert n > 0
    return n


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
R_NB = {0: 300, 1: 301}
R_NQ = 256
R_ABSENT = (0, 10, 63)


def _rows_plan():
    A, B = np.zeros(R_NQ, np.int64), np.zeros(R_NQ, np.int64)
    for p in range(R_NQ):
        a, b = SIZES[p % 8], SIZES[(p // 8) % 8]
        if p // 64 == 1:
            a = 0                                              # block 1: nothing in the lower half
        if p // 64 == 2:
            b = 0                                              # block 2: nothing in the upper half
        if p in R_ABSENT:
            a = b = 0
        A[p], B[p] = a, b
    return A, B


def _rows(form):
    rng = np.random.default_rng(4101)
    A, B = _rows_plan()
    docs = []
    for lst, nb in R_NB.items():
        half = (nb + 1) // 2
        for i in range(nb):
            has = (i < A) if i < half else (i - half < B)
            docs.append(_unit_doc(rng, len(docs), lst, CTL0 + np.flatnonzero(has)))
    allc = CTL0 + np.arange(R_NQ)
    queries = {"full": (allc, _weights(rng, R_NQ)), "part200": (allc[:200], _weights(rng, 200)),
               "thirds": (allc[np.arange(R_NQ) % 3 != 0], _weights(rng, int((np.arange(R_NQ) % 3 != 0).sum()))),
               "one": (allc[65:66], _weights(rng, 1))}
    dots = [(lst, q) for lst in R_NB for q in queries]
    return Case("rows", form, docs, queries, [], UNIT, _check_rows, dots)


def _check_rows(case, ix):
    a = orc.desc_arrays(ix.desc)
    mid = mids(a)
    _unit_blocks(case, a, R_NB)
    comps = case.queries["full"][0]
    assert [_nb(a, case.P(lst)) % 2 for lst in R_NB] == [0, 1] and [_nb(a, case.P(lst)) for lst in R_NB] == list(R_NB.values())
    for lst in R_NB:
        lo, hi = half_lens(a, mid, case.P(lst), comps)
        A, B = _rows_plan()
        assert np.array_equal(lo, A) and np.array_equal(hi, B), lst
        assert set(SIZES) <= set(lo.tolist()) and set(SIZES) <= set(hi.tolist())
        ln = lo + hi
        assert ((lo == 0) & (ln > 0)).any() and ((lo == ln) & (ln > 0)).any()           # mid == 0, mid == len
        for p in R_ABSENT:
            assert ln[p] == 0
        assert ln[9] > 0 and ln[11] > 0 and ln[1] > 0 and ln[62] > 0                    # 10 lies between present rows
        assert (lo[64:128] == 0).all() and (lo[128:192] > 0).any()                      # t_begin == t_end, then a block with work
        assert (hi[128:192] == 0).all() and (hi[192:256] > 0).any()
    v = case.queries["full"][1]
    assert (v < 0).any() and (v > 0).any() and np.abs(v).max() / np.abs(v).min() >= 2.0 ** 20
    assert len(case.queries["part200"][0]) % 64 != 0
    return dict(order_sensitive_accumulators=_order_sensitive(case, a, mid))


# ---------------------------------------------------------------------------------------------------------------------
# chunks
# ---------------------------------------------------------------------------------------------------------------------
C_NB = 300
C_TYPES = (0, 40, 65, 129)           # entries per half of a row of 0, 1, 2, 3 chunks
C_COUNTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


def _chunk_seq(n, rev):
    seq, left = [], n
    for _ in range(64):
        t = min(3, left)
        seq.append(t)
        left -= t
    assert left == 0
    return seq[::-1] if rev else seq


def _chunks(form):
    rng = np.random.default_rng(4202)
    half = (C_NB + 1) // 2
    docs = []
    for i in range(C_NB):
        r = i if i < half else i - half
        docs.append(_unit_doc(rng, len(docs), 0, [CTL0 + 4 * p + t for p in range(64) for t in (1, 2, 3) if r < C_TYPES[t]]))
    queries = {}
    for n in C_COUNTS:
        for rev in (False, True):
            seq = _chunk_seq(n, rev)
            queries["%s%d" % ("r" if rev else "n", n)] = (np.array([CTL0 + 4 * p + t for p, t in enumerate(seq)]), _weights(rng, 64))
    return Case("chunks", form, docs, queries, [], UNIT, _check_chunks, [(0, q) for q in queries])


def _check_chunks(case, ix):
    a = orc.desc_arrays(ix.desc)
    mid = mids(a)
    _unit_blocks(case, a, [0])
    assert _nb(a, case.P(0)) == C_NB
    seen, straddles = set(), 0
    for q, (comps, _) in case.queries.items():
        n = int(q[1:])
        for part in half_lens(a, mid, case.P(0), comps):
            cnt = (part + 63) >> 6
            assert cnt.sum() == n and len(comps) == 64, (q, cnt.sum())
            c0 = np.concatenate([[0], np.cumsum(cnt)])
            if n >= 65:                                          # chunks 63 and 64 belong to the same row
                o63, o64 = np.searchsorted(c0, 63, "right") - 1, np.searchsorted(c0, 64, "right") - 1
                assert o63 == o64, (q, o63, o64)
                straddles += 1
            assert set(part.tolist()) <= set(C_TYPES)
        seen.add(n)
    assert seen == set(C_COUNTS)
    return dict(straddles=straddles, order_sensitive_accumulators=_order_sensitive(case, a, mid))


# ---------------------------------------------------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------------------------------------------------
P_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
P_NB, P_CTL, P_LISTS, P_LIST_NB = 130, 600, (1, 2, 3, 4, 5), 40


def _pairs(form):
    rng = np.random.default_rng(4303)
    docs = []
    for i in range(P_NB):
        docs.append(_unit_doc(rng, len(docs), 0, CTL0 + np.flatnonzero(rng.random(P_CTL) < 0.25)))
    for lst in P_LISTS:
        for i in range(P_LIST_NB):
            docs.append(_unit_doc(rng, len(docs), lst, CTL0 + rng.choice(64, 10, replace=False)))
    queries = {"c%d" % n: (CTL0 + np.sort(rng.choice(P_CTL, n, replace=False)), _weights(rng, n)) for n in P_COUNTS}

    def search_q(n_lists, nnz):
        c = np.concatenate([P_LISTS[:n_lists], CTL0 + rng.choice(64, nnz - n_lists, replace=False)])
        return _sorted_q(c, np.concatenate([8.0 - np.arange(n_lists), _weights(rng, nnz - n_lists, big=False)]))

    queries.update(s4x32=search_q(4, 32), s4x64=search_q(4, 64), s5x64=search_q(5, 64))
    runs = [srun("p128", ("s4x32",), 10, 4, 0.9, dict(qg=4)), srun("p256", ("s4x64",), 10, 4, 0.9, dict(qg=4)),
            srun("p320", ("s5x64",), 10, 5, 0.9, dict(qg=5))]
    return Case("pairs", form, docs, queries, runs, UNIT, _check_pairs, [(0, "c%d" % n) for n in P_COUNTS])


def _check_pairs(case, ix):
    a = orc.desc_arrays(ix.desc)
    mid = mids(a)
    _unit_blocks(case, a, (0,) + P_LISTS)
    assert _nb(a, case.P(0)) == P_NB
    assert [len(case.queries["c%d" % n][0]) for n in P_COUNTS] == list(P_COUNTS)
    for n in P_COUNTS:
        lo, hi = half_lens(a, mid, case.P(0), case.queries["c%d" % n][0])
        assert (lo + hi > 0).sum() >= 0.9 * n and ((lo > 0).any() or n == 1)
    pairs = {}
    for r in case.runs.values():
        q = r.queries[0]
        assert walked(case, q, r.cut) == [case.P(x) for x in P_LISTS[: r.cut]]
        pairs[r.name] = r.cut * len(case.queries[q][0])
        for block in BLOCKS:
            assert hook(case, ix, r, block)["qg"] == r.expect["qg"] == r.cut
    assert pairs == dict(p128=128, p256=256, p320=320)             # NT / 4, NT / 2 at 512 threads; NT / 4 at 1024; and past it
    return dict(pairs=pairs, order_sensitive_accumulators=_order_sensitive(case, a, mid))


# ---------------------------------------------------------------------------------------------------------------------
# directory
# ---------------------------------------------------------------------------------------------------------------------
D_DIM = 65535


def _directory_ids():
    """Four vocabulary ids whose 16 keys (list << 16 | component) put five or more into the LAST of the 7 buckets and five
    or more into another one, and an id absent from the collection whose key with the first list falls into a full bucket."""
    rng = np.random.default_rng(4404)
    nbk = (16 * 10 // 6 + 3) // 4
    for _ in range(200000):
        ids = np.sort(rng.choice(np.arange(1, D_DIM), 4, replace=False))
        home = [row_dir_bucket((int(x) << 16) | int(y), nbk) for x in ids for y in ids]
        cnt = np.bincount(home, minlength=nbk)
        if cnt[nbk - 1] >= 5 and cnt[1: nbk - 1].max() >= 5 and cnt[0] <= 2:
            full = int(np.argmax(cnt[1: nbk - 1])) + 1
            for x in range(1, D_DIM):
                if x not in ids and row_dir_bucket((int(ids[0]) << 16) | x, nbk) == full:
                    return [int(i) for i in ids], x
    raise AssertionError("no ids found")


def _directory(form):
    rng = np.random.default_rng(4405)
    if SC.FORMS[form][0] == 2:
        ids, absent = _directory_ids()
        docs = [(np.array(ids), SC._values(rng, 4)) for _ in range(3)]
        queries = {"all": _sorted_q(ids + [absent], [2.0, -1.5, 1.0, 0.5, 4.0]), "present": _sorted_q(ids, [1.0, 2.0, -0.5, 0.25])}
        runs = [srun("walk", ("all", "present"), 3, 4, 0.0), srun("walk5", ("all", "present"), 3, 5, 0.0)]
        dots = [(c, q) for c in ids for q in queries]
        return Case("directory", form, docs, queries, runs, ONE_FULL, _check_directory_u16, dots, logical_dim=D_DIM)
    docs = [([10], [1.0]), ([20, 25], [1.0, 0.5]), ([30, 35, 38], [1.0, 0.5, 0.25])]
    docs = [(np.array(c), np.array(v, f32)) for c, v in docs for _ in range(3)]
    qc = [5, 10, 15, 20, 22, 25, 27, 30, 33, 35, 36, 38, 39, 40, 45]
    w = np.array([0.5, 3.0, -0.25, 2.5, 0.125, 1.0, -1.0, 2.0, 0.75, 1.25, -0.5, 1.5, 0.375, 3.5, 0.625], f32)
    queries = {"q": (np.array(qc), w), "low": (np.array([1, 2, 3, 40]), np.array([1.0, 2.0, 3.0, 4.0], f32)),
               "high": (np.array([30, 500, 600]), np.array([3.0, 2.0, 1.0], f32))}
    runs = [srun("walk", ("q", "low", "high"), 3, 9, 0.0)]
    dots = [(c, q) for c in (10, 20, 30, 40) for q in queries]
    return Case("directory", form, docs, queries, runs, ONE_FULL, _check_directory_u32, dots)


def _check_directory_u16(case, ix):
    a = orc.desc_arrays(ix.desc)
    tab, nbk = row_dir_table(ix)
    ids = [int(c) for c in case.queries["present"][0]]
    absent = int(np.setdiff1d(case.queries["all"][0], ids)[0])
    assert ix.desc.n_rows == 16 and nbk == 7
    displaced = wrapped = 0
    for x in ids:
        for y in ids:
            key = (x << 16) | y
            e, at = row_dir_lookup(tab, nbk, key)
            assert e is not None
            home = row_dir_bucket(key, nbk)
            displaced += at != home and home != nbk - 1
            wrapped += home == nbk - 1 and at == 0
    key = (ids[0] << 16) | absent
    home = row_dir_bucket(key, nbk)
    assert (tab[home, :, 0] != 0xffffffff).all() and row_dir_lookup(tab, nbk, key)[0] is None      # absent, home bucket full
    assert displaced >= 1 and wrapped >= 1, (displaced, wrapped)
    assert all(_nb(a, c) == 1 for c in ids)
    return dict(displaced=int(displaced), wrapped=int(wrapped), absent=absent)


def _check_directory_u32(case, ix):
    a = orc.desc_arrays(ix.desc)
    assert row_dir_table(ix)[1] == 0
    lrs = a["list_row_start"].astype(np.int64)
    rows = {c: a["row_comp"][lrs[case.P(c)]: lrs[case.P(c) + 1]].astype(np.int64) for c in (40, 10, 20, 30)}
    assert [len(rows[c]) for c in (40, 10, 20, 30)] == [0, 1, 2, 3]
    q = case.queries["q"][0].astype(np.int64)
    for c in (10, 20, 30):
        r = rows[c]
        assert (q < r[0]).any() and (q > r[-1]).any() and np.isin(r, q).all()
    for c in (20, 30):
        assert ((q > rows[c][0]) & (q < rows[c][-1]) & ~np.isin(q, rows[c])).any()                 # between two rows
    assert walked(case, "q", 9)[0] == case.P(40) and case.P(40) in walked(case, "low", 9)           # the list without rows is walked
    assert case.queries["low"][0].max() == case.P(40) and (case.queries["high"][0][1:] > rows[30][-1]).all()
    return dict(rows={c: len(r) for c, r in rows.items()})


# ---------------------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------------------
G_NB = (40, 30, 50, 0, 20, 35, 10, 25, 15)      # blocks of lists 0 .. 8, the order they are walked in


def _groups(form):
    rng = np.random.default_rng(4506)
    docs = []
    for lst, nb in enumerate(G_NB):
        for _ in range(nb):
            docs.append(_unit_doc(rng, len(docs), lst, CTL0 + rng.choice(20, 3, replace=False)))
    c = np.concatenate([np.arange(9), CTL0 + np.arange(6)])
    queries = {"nine": _sorted_q(c, np.concatenate([9.0 - np.arange(9), [0.5, -0.25, 0.125, 0.375, -0.75, 0.0625]])),
               "other": _sorted_q(c[:12], np.concatenate([9.0 - np.arange(9), [0.25, -0.5, 0.125]]))}
    qs = ("nine", "other")
    runs = []
    for cut in (7, 9):
        runs += [srun("lg%d_c%d" % (lg, cut), qs, 10, cut, 0.9, dict(qg=lg), env=dict(SGPU_LIST_GROUP=str(lg))) for lg in (1, 2, 3)]
        runs += [srun("cap%d_c%d" % (cap, cut), qs, 10, cut, 0.9, dict(dots_cap=cap), env=dict(SGPU_DOTS_CAP=str(cap)))
                 for cap in (G_NB[0] + G_NB[1], G_NB[0] + G_NB[1] - 1)]
    runs += [srun("free9", qs, 10, 9, 0.9, dict(qg=9)), srun("free5", qs, 10, 5, 0.9, dict(qg=5))]
    return Case("groups", form, docs, queries, runs, UNIT, _check_groups)


def _check_groups(case, ix):
    a = orc.desc_arrays(ix.desc)
    _unit_blocks(case, a, [i for i, nb in enumerate(G_NB) if nb])
    assert [_nb(a, case.P(i)) for i in range(9)] == list(G_NB)
    found = {}
    for q in ("nine", "other"):
        assert walked(case, q, 9) == [case.P(i) for i in range(9)]
    for r in case.runs.values():
        for block in BLOCKS:
            h = hook(case, ix, r, block)
            for k_, v_ in r.expect.items():
                assert h[k_] == v_, (r.name, block, k_, h[k_])
            found[r.name] = plan_groups(G_NB[: r.cut], h["dots_cap"], h["qg"])
    assert found["lg1_c9"] == [[i] for i in range(9)] and found["lg2_c7"] == [[0, 1], [2, 3], [4, 5], [6]]
    assert found["lg3_c9"] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]] and found["lg3_c7"][-1] == [6]
    assert found["cap70_c9"] == [[0, 1], [2, 3, 4], [5, 6, 7], [8]]          # 40 + 30 == 70: equality; the empty list inside a group
    assert found["cap69_c9"] == [[0], [1], [2, 3], [4, 5, 6], [7, 8]]
    assert found["cap70_c7"] == [[0, 1], [2, 3, 4], [5, 6]]
    assert found["free9"] == [list(range(9))] and found["free5"] == [list(range(5))]
    assert 2 * 9 > 1024 // 64 and 2 * 5 > 512 // 64                            # more streams than wavefronts
    return found


# ---------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------
S_LISTS, S_DIM = 12, 2000


def _select(form):
    rng = np.random.default_rng(4607)
    docs = []
    for lst in range(S_LISTS):
        for _ in range(30):
            c = np.concatenate([[lst], np.sort(rng.choice(np.arange(1200, S_DIM), 3, replace=False))])
            docs.append((c, SC._values(rng, 4)))
    queries = {"eq600": (np.arange(2, 602), np.full(600, 0.5, f32)), "eq1100": (np.arange(1, 1101), np.full(1100, 0.5, f32)),
               "tie": (np.arange(8), np.array([3, 3, 2, 2, 1, 1, 1, 0.5], f32)),
               "tie_rev": (np.arange(8), np.array([0.5, 1, 1, 1, 2, 2, 3, 3], f32)),
               "neg": (np.arange(6), np.array([2.0, -1.0, 0.0, -3.0, 1.0, 0.5], f32))}
    runs = [srun("eq_cut%d" % cut, ("eq600", "eq1100"), 10, cut, 0.9) for cut in (1, 5, 8)]
    runs += [srun("tie_cut%d" % cut, ("tie", "tie_rev"), 10, cut, 0.9) for cut in (1, 3, 5, 6)]
    runs += [srun("neg_cut%d" % cut, ("neg",), 10, cut, 0.9) for cut in (0, 1, 5, 6, 7)]
    return Case("select", form, docs, queries, runs, ONE, _check_select, logical_dim=S_DIM)


def _check_select(case, ix):
    a = orc.desc_arrays(ix.desc)
    assert all(_nb(a, case.P(i)) == 1 for i in range(S_LISTS))
    assert len(case.queries["eq600"][0]) == 600 > 512 and len(case.queries["eq1100"][0]) == 1100 > 1024
    assert walked(case, "eq600", 5) == [case.P(i) for i in range(2, 7)] and walked(case, "eq1100", 8) == [case.P(i) for i in range(1, 9)]
    for cut in (1, 3, 5):                                                     # an equal pair on either side of the cut
        v = np.sort(case.queries["tie"][1])[::-1]
        assert v[cut - 1] == v[cut]
    assert walked(case, "tie", 3) == [case.P(i) for i in (0, 1, 2)] and walked(case, "tie_rev", 3) == [case.P(i) for i in (6, 7, 4)]
    assert walked(case, "neg", 6) == [case.P(i) for i in (0, 4, 5, 2, 1, 3)]
    assert {r.cut for r in case.runs.values() if r.queries == ("neg",)} == {0, 1, 5, 6, 7} and len(case.queries["neg"][0]) == 6
    model = M64.Model(a, ix.desc.val_scale, ix.desc.value_type)
    for r in case.runs.values():
        got = SC.counts(case, ix.desc, r)
        for q in r.queries:
            w = walked(case, q, r.cut)
            assert got[q]["blocks_total"] == sum(_nb(a, c) for c in w), (r.name, q)
            assert [int(x) for x in model.selected_lists(model.query(*case.queries[q]), r.cut)] == w
    return dict(walked_tie_rev=walked(case, "tie_rev", 3))


# ---------------------------------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------------------------------
L_DIMS = (992, 1023, 997, 998)        # dim % 4 = 0, 3, 1, 2; dim % 32 = 0, 31
L_CYCLE = 1099                        # 7 x 157 queries: more than the chip keeps workgroups resident
L_POOL = ("long", "short", "plain", "scaled", "last", "words", "empty")
L_LAYOUTS = {"u16_f16": (("dense", {}), ("packed", dict(SGPU_NO_DENSE="1"))),
             "u16_u8": (("dense", {}), ("packed", dict(SGPU_NO_DENSE="1"))),
             "u32_f16": (("hashed", dict(SGPU_FORCE_HASH="1")), ("packed", dict(SGPU_NO_HASH="1")),
                         ("split", dict(SGPU_NO_HASH="1", SGPU_FORCE_SPLIT="1")))}
L_WORDS = (128, 159, 160, 191)


def _lookup(form, tag):
    D = int(tag)
    rng = np.random.default_rng(4708 + D)
    cw = SC.FORMS[form][0]
    dim = D if cw == 2 else next(U32_BASE + 70 * D - r for r in range(70) if (70 * D - r) % 32 == D % 32)
    words = [w for w in L_WORDS] if cw == 2 else [128, 144, 160, 176]          # (u32 ids are multiples of 70: word firsts only)
    docs = []
    for lst in range(6):
        for i in range(50):
            body = rng.choice(np.arange(200, D - 1), int(rng.integers(8, 41)), replace=False)
            extra = ([D - 1] if i % 3 == 0 else []) + ([words[(i // 2) % 4]] if i % 2 else [])
            c = np.unique(np.concatenate([[lst], body, extra]).astype(np.int64))
            docs.append((c, SC._values(rng, len(c))))

    def q(heads, n_body, pool, extra=()):
        c = np.concatenate([np.asarray(heads), rng.choice(pool, n_body, replace=False), np.asarray(extra, np.int64)]).astype(np.int64)
        v = np.concatenate([3.0 - 0.25 * np.arange(len(heads)), (np.arange(n_body + len(extra)) + 1) / 256.0])
        return _sorted_q(c, v)

    lowp, highp = np.arange(200, 600), np.arange(600, D - 1)
    queries = {"long": q([0, 1], 253, lowp), "short": q([2, 3], 3, highp), "plain": q([4, 0], 98, lowp), "scaled": q([5, 2], 18, highp),
               "last": q([1, 3], 5, lowp, [D - 1]), "words": q([5], 0, lowp, words), "empty": SC.EMPTY_Q}
    runs = [srun("%s_%s" % (lname, "coop" if coop else "plain"), L_POOL, 10, 3, 0.9, dict(lookup=LOOKUP[lname]), coop=coop, env=env,
                 cycle=L_CYCLE) for lname, env in L_LAYOUTS[form] for coop in (False, True)]
    return Case("lookup", form, docs, queries, runs, dict(ONE, n_postings=400), _check_lookup, logical_dim=D, dim=dim, tag=tag)


def _check_lookup(case, ix):
    D, dim = case.logical_dim, case.dim
    assert ix.desc.dim == dim and dim % 32 == D % 32 and dim % 4 == D % 4 and D in L_DIMS
    a = orc.desc_arrays(ix.desc)
    assert _nb(a, dim - 1) >= 1 and (a["fwd_comps"] == dim - 1).sum() >= 50          # documents hold dim - 1
    Q = case.queries
    assert len(Q["long"][0]) == 255 and len(Q["short"][0]) == 5 and not np.isin(Q["short"][0], Q["long"][0]).any()
    assert len(Q["plain"][0]) > 63 >= len(Q["scaled"][0]) and (dim - 1) in Q["last"][0]
    w = Q["words"][0].astype(np.int64)
    assert (w % 32 == 0).any() and (case.cw == 4 or (w % 32 == 31).any()) and np.isin(w, a["fwd_comps"]).all()
    if dim % 32 == 0:
        assert (dim - 1) % 32 == 31
    pool = L_POOL
    assert pool.index("short") == pool.index("long") + 1 and pool.index("scaled") == pool.index("plain") + 1
    assert L_CYCLE % len(pool) == 0 and L_CYCLE > 2 * 512
    layouts = {}
    for r in case.runs.values():
        # a forced-hash run is hashed only if EVERY query of its batch has a collision-free seed (hash_cases.py restates the
        # search): every query of L_POOL has seed 0 here - ids that are multiples of 70 spread well - so no run of this case
        # falls back and none needs a sibling batch; test_gpu_stage01_edges.py asserts the lookup that ran through the lane hook
        ok = H.seeds(*case.batch(r)[:2], case.dim, case.cw, case.value_type, "SGPU_NO_HASH" in knob_env(case, r, 512))[0]
        assert ok == ("SGPU_FORCE_HASH" in r.env), (r.name, ok)
        for block in BLOCKS:
            h = hook(case, ix, r, block, hash_ok=ok)
            assert h["lookup"] == r.expect["lookup"], (r.name, block, h["lookup"])
            assert (h["coop"] != 0) == r.coop and (h["streamed"] == 1) == (not r.coop), (r.name, h)
            layouts[r.name] = h["lookup"]
    return layouts


# ---------------------------------------------------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------------------------------------------------
T_NB = (2, 3, 64, 65, 512, 513, 1025, 2049)


def _sort(form):
    rng = np.random.default_rng(4809)
    docs = []
    for lst, nb in enumerate(T_NB):
        for i in range(nb):
            g = i // 4                                              # runs of four documents equal in the queried components
            docs.append(_unit_doc(rng, len(docs), lst, [CTL0 + lst], [(g * 5 % 13 + 1) / 64.0], lst_val=(g * 7 % 29 + 1) / 64.0))
    queries = {"s%d" % nb: (np.array([lst, CTL0 + lst]), np.array([1.0, -0.75], f32)) for lst, nb in enumerate(T_NB)}
    names = tuple(queries)
    runs = [srun("sorted", names, 5, 1, 1.0, first_sorted=True), srun("unsorted", names, 5, 1, 1.0),
            srun("sorted_k2", names, 2, 1, 1.0, first_sorted=True)]
    return Case("sort", form, docs, queries, runs, UNIT, _check_sort, [(lst, "s%d" % nb) for lst, nb in enumerate(T_NB)])


def _check_sort(case, ix):
    a = orc.desc_arrays(ix.desc)
    _unit_blocks(case, a, range(len(T_NB)))
    assert [_nb(a, case.P(i)) for i in range(len(T_NB))] == list(T_NB)
    for wg in BLOCKS:                                               # n2 / 2 below, at and above the workgroup size
        n2 = [1 << int(np.ceil(np.log2(nb))) for nb in T_NB]
        assert any(x // 2 < wg for x in n2) and any(x // 2 == wg for x in n2) and any(x // 2 > wg for x in n2), wg
    ties = negative = 0
    for lst, nb in enumerate(T_NB):
        d = orc.summary_distances(ix.desc, case.P(lst), *case.queries["s%d" % nb])
        assert len(d) == nb
        ties += int(nb - len(np.unique(d)))
        negative += int((d < 0).sum())
        if nb >= 64:
            assert (np.diff(d) != 0).any() and (d[:4] == d[0]).all()
    assert ties > 100 and negative > 10
    s, u = (orc.batch_search_counts(ix.desc, *case.batch(case.runs[n]), 5, 1, 1.0, n == "sorted") for n in ("sorted", "unsorted"))
    differ = [i for i in range(len(T_NB)) if not np.array_equal(s[3][i], u[3][i]) or not np.array_equal(s[1][i], u[1][i])]
    assert len(differ) >= 4, differ
    return dict(ties=ties, negative=negative, queries_that_differ=differ)


# ---------------------------------------------------------------------------------------------------------------------
KINDS = {"rows": (_rows, ("u16_f16", "u32_f16")), "chunks": (_chunks, ("u16_f16", "u32_f16")), "pairs": (_pairs, ("u16_f16", "u32_f16")),
         "directory": (_directory, ("u16_f16", "u32_f16")), "groups": (_groups, ("u16_f16", "u32_f16")),
         "select": (_select, ("u16_f16", "u32_f16")), "sort": (_sort, ("u16_f16", "u32_f16"))}
LOOKUP_NAMES = tuple("lookup-%s-%d" % (f, d) for f, ds in (("u16_f16", L_DIMS), ("u16_u8", L_DIMS[:2]), ("u32_f16", L_DIMS[:2])) for d in ds)
CASE_NAMES = tuple("%s-%s" % (k, f) for k, (_, forms) in KINDS.items() for f in forms) + LOOKUP_NAMES
DOT_CASES = tuple(n for n in CASE_NAMES if n.split("-")[0] in ("rows", "chunks", "pairs", "directory"))
WALK_CASES = tuple(n for n in CASE_NAMES if n.split("-")[0] in ("rows", "chunks", "pairs"))
SEARCH_CASES = tuple(n for n in CASE_NAMES if n.split("-")[0] in ("pairs", "directory", "groups", "select", "lookup", "sort"))


@functools.lru_cache(maxsize=None)
def make(name):
    """The case `name` = "<kind>-<form>[-<dim>]" (built once per process; its arrays are read-only)."""
    kind, form, *tag = name.split("-")
    return _lookup(form, tag[0]) if kind == "lookup" else KINDS[kind][0](form)
