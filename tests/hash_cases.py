"""Seeded inputs and the restatement for the tests of the hashed query lookup (LK_HASH, sk_u32_hash.hip; u32 components, f16
values): test_hash_cases_cpu.py, test_gpu_hash_lookup.py. TEST INFRASTRUCTURE, pure numpy apart from the index build.

hash_mult(), hash_slot() and seeds() restate, from the text of device_types.hpp (hash_mult, hash_slot) and launch_plan.hip
(make_plan: "LK_HASH seeds") alone, in Python integers:

  multiplier   (((seed + 1) * 2654435761) >> 8 | 1) & 0xffffff: bits 8 ... 31 of the product, forced odd - 24 bits
  slot         the top 12 bits of the LOW 32 bits of (component & 0xffffff) * multiplier: a table of 4096 slots
  seed         per query, the FIRST of the 64 seeds whose multiplier sends the query's components to distinct slots; a query
               of more than 4096 / 4 = 1024 components has none, whatever its ids
  hash_ok      u32 components, f16 values, dim < 2^24, no SGPU_NO_HASH, and EVERY query of the batch has a seed; the search
               stops at the first query without one (its entry and all later entries read 0)

One switch per wrong reading (WRONG); check() shows on the CPU that each changes the answer on a named case:
  even_mult     the multiplier is not forced odd                              -> `odd` (found by search for it)
  wide_mult     the multiplier keeps the product's bits above 31              -> `seed1` (seed 0's product has none)
  top_bits      the slot is bits 52 ... 63 of the 64-bit product (always 0)     -> `eight`
  wide_comp     the component is not masked to 24 bits: only ids >= 2^24 can tell, which is WHY hash_ok asks for
                dim < 2^24 - the device multiplies with __umul24, which sees 24 bits -> WIDE_IDS (no index holds them)
  strict_limit  `< 1024` for `<= 1024`                                        -> `fill1024`
  last_seed     the last collision-free seed instead of the first             -> `eight`
  skip_failed   a query without a seed is skipped, the batch stays hashed     -> `mixed`

Two collections of N_DOCS + N_MATES documents, u32 components, f16 values, named by their vocabulary:
  small  dim 70 000
  large  dim 2^24 - 1 = 16 777 215, the largest vocabulary the hashed lookup takes. Its body ids lie in [0, 2^16),
         [2^16, 2^20), [2^20, 2^24) and 200 of them at 0xf00000 and above (bits 20 - 23 all set); dim - 1 is a list.
Build times measured on the CPU (8 threads, these documents, the builder alone): dim 70 000 0.07 s, dim 2^20 - 1 0.6 s,
dim 2^24 - 1 8 s, dim 2^24 5 s (BUILD_SECONDS) - several per-component arrays scale with dim. 2^24 - 1 is the only vocabulary
whose sentinel id is 0xffffff and whose ids fill all 24 bits the device's multiply sees, so it is kept although it is the slow
one: it is built once per process and shared by every test. dim == 2^24 (`wide`, the same documents) is built for ONE case:
hash_ok == 0.
NO FALLBACK FITS THE LARGE VOCABULARY: the packed lookup needs 8 bytes and the split one 6 per 32 ids - 4 MB and 3 MB of
LDS at dim 2^24 - 1 (the limit is 160 KB: u32 vocabularies above ~650 000 ids can be searched through the hashed lookup
only). Two things follow, and they are not alike:
  THE LIMIT   a batch of `large` that holds a query WITHOUT a seed (`mixed`, `rule`) cannot be searched: SGPU_ELIMIT, from
              the launch-configuration hook and from the launch alike. That is a capacity limit; the tests assert it, and
              the fallback layouts are walked on `small`.
  THE DEFECT these cases found, fixed with them: `alone_fit` on `large` - every query seeded - ALSO failed with SGPU_ELIMIT.
              launch_configure declined the hashed table because it did not fit the 80 KB two workgroups share a CU on -
              an occupancy preference - and then had no layout left, although the launch fits the 160 KB limit (99.6 KB).
              It now keeps the hashed table when no fallback layout fits the limit and the hashed one does: `alone_fit`
              on `large` reports lookup == 3 and returns the oracle's rows.

Queries (found by seeded search; check() asserts what each is there for):
  sizes      empty, one, eight: 0, 1 and 8 components
  fill edge  fill1024: the 1024 consecutive ids from FILL0 on - seed 0, the table exactly a quarter full;
             fill1025: 1025 of them - no seed, by the rule
  seeds      seed1 (first seed 1), c2, c3, c5 (first seeds 2, 3, 5), seed16p (first seed >= 16), seedmax: the highest first
             seed among SEEDMAX_TRIES random queries of 128 ... 160 components (SEED_FOUND records both)
  failure    fail300: 300 random components, no seed
  large ids  big16 (ids >= 2^16), big20 (ids >= 2^20; large), last (holds dim - 1)
  slot-mates mates: see mate_documents()
  weights    neg: negative weights and one -0.0
  odd        a query whose first seed changes when the multiplier is not forced odd
Slot-mates. Under the multiplier of `mates`, the N_MATES last documents each store 1 - 3 components that are NOT in the query
but share a slot with one that is, next to components that are; half of them have a length that is no multiple of 8, and
`mates` holds a component chosen so that the padding sentinel `dim` of such records shares ITS slot. A kernel that dropped
the id compare would give the slot's weight to the slot-mate: wrong_score() computes that score in numpy, check() asserts
that it differs from the float64 score of every mate document by more than the f32 bound. (A sentinel's value is +0.0, so
the product it would add is +-0.0: the sentinel alone cannot change a score, which is why every sentinel document also
stores a slot-mate.)

Batches (Run): sizes, cycle (seven queries of seven different seeds over CYCLE queries: every persistent workgroup changes
multiplier between consecutive queries), mixed (the same plus fail300: the whole batch falls back), alone (fill1024 under
SGPU_FORCE_HASH: the row tables of a 1024-component query and the 32 KB table together pass the 80 KB a workgroup may take
when two share a CU, so the LDS fitting of launch_configure DECLINES the hashed lookup for it where another layout fits -
alone_fit on `small` is that launch, the one named case of a seeded batch that is not hashed; on `large` nothing else fits
and alone_fit is hashed - and the forced launch takes 99.6 KB), rule (fill1025: falls back), mates (k = 200, heap_factor
0: every mate document is in the row).
LDS_DECLINES names the (vocabulary, batch) pairs whose every query has a seed and whose launch is still not hashed.
"""
import functools

import numpy as np

import model64 as M64
import orc
import stream_cases as SC
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

f32 = np.float32
HASH_BITS, HASH_SLOTS, HASH_SEEDS = 12, 4096, 64       # device_types.hpp: kHashBits, kHashSlots, kHashSeeds
LK_HASH = 3
WRONG = ("even_mult", "wide_mult", "top_bits", "wide_comp", "strict_limit", "last_seed", "skip_failed")
DIMS = {"small": 70000, "large": (1 << 24) - 1, "wide": 1 << 24}
VOCABS = ("small", "large")
BUILD_SECONDS = {"small": 0.07, "large": 8.0, "wide": 5.0}
N_DOCS, N_MATES, N_HEADS, N_POOL = 2000, 64, 12, 600
FILL0 = 1000                                            # fill1024 = ids [FILL0, FILL0 + 1024)
CYCLE_POOL = ("seedmax", "c2", "seed1", "c3", "seed16p", "mates", "c5")
CYCLE = 2100                                            # 7 x 300: more queries than the chip keeps workgroups resident
SEEDMAX_TRIES = 400
SEED_FOUND = {"small": dict(seed16p=20, seedmax=58), "large": dict(seed16p=26, seedmax=61)}   # (check() asserts them)
WIDE_IDS = np.array([(1 << 24) + 5, (3 << 24) + 5, 5, (1 << 24) + 4101], np.int64)            # the `wide_comp` case
CFG = dict(n_postings=400, centroid_fraction=0.1, summary_energy=0.5, max_fraction=2.0, min_cluster_size=2, doc_cut=10)
LDS_DECLINES = (("small", "alone_fit"),)
KNN = 3                                                 # neighbours per document of the graph the kNN run uses


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def hash_mult(seed, wrong=None):
    m = ((int(seed) + 1) * 2654435761) >> 8
    if wrong != "wide_mult":
        m &= 0xffffff                                   # (u32 arithmetic: the product's bits 8 ... 31)
    return m if wrong == "even_mult" else m | 1


def hash_slot(c, mult, wrong=None):
    """Slots of components c (any integer array) under one multiplier."""
    c = np.asarray(c, np.int64).astype(np.uint64)      # (ids < 2^32 and multipliers < 2^39: every product fits 64 bits)
    if wrong != "wide_comp":
        c = c & np.uint64(0xffffff)
    p = c * np.uint64(mult)
    s = p >> np.uint64(52) if wrong == "top_bits" else (p & np.uint64(0xffffffff)) >> np.uint64(32 - HASH_BITS)
    return s.astype(np.int64)


def query_seed(comps, wrong=None):
    """A query's seed, or HASH_SEEDS where it has none."""
    n = len(comps)
    if n >= HASH_SLOTS // 4 if wrong == "strict_limit" else n > HASH_SLOTS // 4:
        return HASH_SEEDS
    found = HASH_SEEDS
    for s in range(HASH_SEEDS):
        if len(np.unique(hash_slot(comps, hash_mult(s, wrong), wrong))) == n:
            found = s
            if wrong != "last_seed":
                break
    return found


def seeds(q_off, comps, dim, comp_width=4, value_type=0, no_hash=False, wrong=None):
    """(hash_ok, per-query entries) of a batch as make_plan computes them: the loop stops at the first query without a seed."""
    q_off = np.asarray(q_off, np.int64)
    nq = len(q_off) - 1
    out = np.zeros(nq, np.uint32)
    ok = dim < (1 << 24) and comp_width == 4 and value_type == 0 and not no_hash
    if not ok:
        return 0, out
    for q in range(nq):
        s = _seed_cached(np.asarray(comps[q_off[q]: q_off[q + 1]], np.uint32).tobytes(), wrong)
        if s == HASH_SEEDS:
            if wrong == "skip_failed":
                continue
            return 0, out
        out[q] = s
    return 1, out


@functools.lru_cache(maxsize=None)
def _seed_cached(raw, wrong):
    return query_seed(np.frombuffer(raw, np.uint32), wrong)


def wrong_score(qc, qv, dc, dv, dim):
    """The float64 score of a document (components dc, values dv) that a kernel WITHOUT the id compare would give under the
    query's multiplier: every element takes the weight of whatever query component sits in its slot; the record's padding
    (sentinel id `dim`, value +0.0) is scored like any element."""
    mult = hash_mult(query_seed(qc))
    table = np.zeros(HASH_SLOTS, np.float64)
    table[hash_slot(qc, mult)] = np.asarray(qv, np.float64)
    npad = -len(dc) % 8
    c = np.concatenate([np.asarray(dc, np.int64), np.full(npad, dim, np.int64)])
    v = np.concatenate([np.asarray(dv, np.float64), np.zeros(npad)])
    return float((table[hash_slot(c, mult)] * v).sum())


def right_score(qc, qv, dc, dv):
    """(float64 score, the f32 bound gamma(m + 1) * sum |q v| of model64) of a document from the forward arrays."""
    w = dict(zip((int(x) for x in qc), (float(x) for x in np.asarray(qv, np.float64))))
    p = np.array([w.get(int(c), 0.0) * float(v) for c, v in zip(dc, dv)], np.float64)
    m = sum(int(c) in w for c in dc)
    return float(p.sum()), float(M64.gamma(m + 1) * np.abs(p).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the collections
# ---------------------------------------------------------------------------------------------------------------------
def _vocabulary(vocab):
    """(heads, pool): the list components and the body components in use, by vocabulary."""
    dim = DIMS[vocab]
    rng = np.random.default_rng(7100 + len(vocab))
    heads = [FILL0 + 5 + 70 * i for i in range(8)]
    if vocab == "small":
        heads += [65536 + 3, 66000, 69000, dim - 1]
        ranges = [(0, FILL0, 100), (FILL0, FILL0 + 1025, 100), (FILL0 + 1025, 65536, 200), (65536, dim - 1, 200)]
    else:
        heads += [65536 + 3, (1 << 20) + 5, 0xf00001, dim - 1]
        ranges = [(0, FILL0, 50), (FILL0, FILL0 + 1025, 100), (FILL0 + 1025, 65536, 50), (65536, 1 << 20, 100),
                  (1 << 20, 0xf00000, 100), (0xf00000, (1 << 24) - 2, 200)]
    pool = np.concatenate([rng.choice(np.setdiff1d(np.arange(lo, hi) if hi - lo < 200000 else np.unique(rng.integers(lo, hi, 4000)),
                                                   heads), n, replace=False) for lo, hi, n in ranges])
    assert len(pool) == N_POOL == len(np.unique(pool))
    return np.array(heads, np.int64), np.sort(pool).astype(np.int64)


def _sorted(c, v):
    o = np.argsort(np.asarray(c, np.int64), kind="stable")
    assert len(np.unique(c)) == len(c)
    return np.asarray(c, np.int64)[o], np.asarray(v, f32)[o]


def _random_query(rng, heads, pool, n):
    """n components: two lists (weights 3.0, 2.0) and body components with small distinct weights."""
    h = rng.choice(heads, min(2, n), replace=False)
    body = rng.choice(pool, n - len(h), replace=False)
    return _sorted(np.concatenate([h, body]), np.concatenate([[3.0, 2.0][: len(h)], (rng.permutation(len(body)) + 1) / 256.0]))


def _find(rng, heads, pool, lo, hi, want, tries=20000):
    for _ in range(tries):
        q = _random_query(rng, heads, pool, int(rng.integers(lo, hi + 1)))
        if want(query_seed(q[0])):
            return q
    raise AssertionError("no query found")


def _find_pair(rng, heads, pool, lo, hi, want, tries=20000):
    for _ in range(tries):
        q = _random_query(rng, heads, pool, int(rng.integers(lo, hi + 1)))
        if want(q[0]):
            return q
    raise AssertionError("no query found")


def _mates_query(rng, heads, pool, dim, taken):
    """The `mates` query: lists heads[0] (4.0) and heads[1] (3.0), 30 body components, and the component that shares the
    padding sentinel's slot (weight 2.5); its seed is none of `taken`."""
    for _ in range(20000):
        body = rng.choice(pool, 30, replace=False)
        c = np.concatenate([heads[:2], body])
        s = query_seed(c)
        if s == HASH_SEEDS or s in taken:
            continue
        mult = hash_mult(s)
        sent = int(hash_slot([dim], mult)[0])
        if sent in hash_slot(c, mult):
            continue
        xs = np.arange(FILL0 + 2000, min(dim, FILL0 + 60000))
        xs = xs[(hash_slot(xs, mult) == sent) & ~np.isin(xs, c) & ~np.isin(xs, heads)]
        if len(xs):                                       # the smallest id from there on that hashes to the sentinel's slot
            x = int(xs[0])
            q = _sorted(np.concatenate([c, [x]]), np.concatenate([[4.0, 3.0], (np.arange(30) + 1) / 64.0, [2.5]]))
            assert query_seed(q[0]) == s                  # (a superset: the earlier seeds still clash, this one still does not)
            return q, x
    raise AssertionError("no mates query found")


def mate_documents(rng, q, dim, heads, sent_comp):
    """N_MATES documents on list heads[0] (value 8.0 and up: each is in the top 200): some of the query's components, 1 - 3
    SLOT-MATES (ids not in the query that share a slot with a query component of weight >= 0.25) and, every other one, the
    sentinel's slot-mate `sent_comp` itself; lengths 5 ... 23, half of them no multiple of 8."""
    qc, qv = q
    mult = hash_mult(query_seed(qc))
    slot_of = {int(s): int(c) for c, s in zip(qc, hash_slot(qc, mult))}
    heavy = [int(c) for c, v in zip(qc, qv) if v >= 0.25 and c != heads[0]]
    mates = {}
    x = FILL0 + 3000
    while len(mates) < 12:                                # one slot-mate id for each of 12 heavy query components
        s = int(hash_slot([x], mult)[0])
        if s in slot_of and slot_of[s] in heavy and slot_of[s] not in mates and x not in qc and x not in heads and x < dim:
            mates[slot_of[s]] = x
        x += 1
    ids = list(mates.values())
    docs = []
    lengths = (5, 8, 9, 16, 12, 24, 15, 8, 17, 16, 23, 24)
    for i in range(N_MATES):
        n = lengths[i % len(lengths)]
        m = [ids[(i + j) % len(ids)] for j in range(1 + i % 3)]
        own = [int(c) for c in rng.choice(qc[qc != heads[0]], 2, replace=False) if c != sent_comp]
        c = [int(heads[0])] + m + own + ([sent_comp] if i % 2 else [])
        fill = [int(y) for y in rng.choice(np.arange(FILL0 + 5000, FILL0 + 9000), 40, replace=False) if y not in c and y not in qc]
        c = np.array((c + fill)[:n] if len(c) < n else c[:n], np.int64)
        assert len(np.unique(c)) == len(c) == n and np.isin(m[0], c)
        v = (rng.integers(32, 256, n) / 64.0).astype(f32)
        v[c == heads[0]] = 8.0 + (i % 8) / 16.0
        docs.append(_sorted(c, v))
    return docs, mates


class HashCase:
    """A collection, its named queries and its batches (stream_cases.Run). It has what stream_cases.plan_facts and
    FilteredDesc read of a case - cw, value_type, dim, allowed() - and nothing else of a StreamCase."""
    form = "u32_f16"

    def __init__(self, vocab):
        self.vocab, self.kind, self.name = vocab, "hash", "hash-" + vocab
        self.cw, self.value_type = SC.FORMS[self.form]
        self.dim = DIMS[vocab]
        src = "large" if vocab == "wide" else vocab        # (`wide`: the documents and queries of `large`)
        d = DIMS[src]
        heads, pool = _vocabulary(src)
        self.heads, self.pool = heads, pool
        rng = np.random.default_rng(7200 + len(src))
        Q = {"empty": SC.EMPTY_Q, "one": _sorted([heads[0]], [1.0]),
             "eight": _sorted(np.concatenate([heads[2:4], pool[::80][:6]]), [3.0, 2.0, 0.5, 0.25, 0.75, 0.125, 1.0, 0.375]),
             "fill1024": (np.arange(FILL0, FILL0 + 1024), ((np.arange(1024) * 37 % 1024 + 1) / 512.0).astype(f32)),
             "fill1025": (np.arange(FILL0, FILL0 + 1025), ((np.arange(1025) * 37 % 1025 + 1) / 512.0).astype(f32))}
        for name, s in (("seed1", 1), ("c2", 2), ("c3", 3), ("c5", 5)):
            Q[name] = _find(rng, heads, pool, 90, 120, lambda x, s=s: x == s)
        Q["odd"] = _find_pair(rng, heads, pool, 90, 120, lambda q: query_seed(q, "even_mult") != query_seed(q) < HASH_SEEDS)
        Q["seed16p"] = _find(rng, heads, pool, 128, 160, lambda x: 16 <= x < HASH_SEEDS)
        tries = [_random_query(rng, heads, pool, int(rng.integers(128, 161))) for _ in range(SEEDMAX_TRIES)]
        found = [query_seed(q[0]) for q in tries]
        self.seedmax_share = float(np.mean([s < HASH_SEEDS for s in found]))
        Q["seedmax"] = tries[int(np.argmax([s if s < HASH_SEEDS else -1 for s in found]))]
        Q["fail300"] = _find(rng, heads, pool, 300, 300, lambda x: x == HASH_SEEDS)
        taken = {query_seed(Q[n][0]) for n in CYCLE_POOL if n in Q}
        Q["mates"], self.sent_comp = _mates_query(rng, heads, pool, d, taken)
        big = pool[pool >= 65536]
        Q["big16"] = _sorted(np.concatenate([[heads[8]], rng.choice(big, 20, replace=False)]), np.concatenate([[2.0], (np.arange(20) + 1) / 32.0]))
        if src == "large":
            big = pool[pool >= 1 << 20]
            Q["big20"] = _sorted(np.concatenate([heads[9:11], rng.choice(big, 40, replace=False)]), np.concatenate([[2.0, 1.5], (np.arange(40) + 1) / 64.0]))
        Q["last"] = _sorted(np.concatenate([heads[10:12], rng.choice(pool, 10, replace=False)]), np.concatenate([[1.0, 2.0], (np.arange(10) + 1) / 16.0]))
        c = np.concatenate([heads[4:6], rng.choice(pool, 18, replace=False)])
        Q["neg"] = _sorted(c, np.concatenate([[2.0, -1.0], -(np.arange(17) + 1) / 8.0, [-0.0]]))
        docs = []
        for i in range(N_DOCS):
            body = rng.choice(pool, int(rng.integers(5, 41)), replace=False)
            docs.append(_sorted(np.concatenate([[heads[i % N_HEADS]], body]), (rng.integers(1, 256, len(body) + 1) / 64.0).astype(f32)))
        self.mate_docs, self.mate_ids = mate_documents(rng, Q["mates"], d, heads, self.sent_comp)
        docs += self.mate_docs
        self.n_docs, self.cfg, self.logical_dim = len(docs), CFG, self.dim
        self.off, self.comps, self.vals = orc.csr(docs)
        self.queries = {n: (np.asarray(c, np.uint32), np.asarray(v, f32)) for n, (c, v) in Q.items()}
        sizes = ("empty", "one", "eight", "odd", "neg", "big16") + (("big20",) if "big20" in Q else ()) + ("last",)
        runs = [SC.Run("sizes", sizes, 10, 3, 0.9), SC.Run("cycle", CYCLE_POOL, 10, 3, 0.8, cycle=CYCLE),
                SC.Run("mixed", CYCLE_POOL + ("fail300",), 10, 3, 0.8, cycle=CYCLE // 7 * 8),
                SC.Run("alone", ("fill1024",), 10, 2, 0.9, env=dict(SGPU_FORCE_HASH="1")), SC.Run("alone_fit", ("fill1024",), 10, 2, 0.9),
                SC.Run("rule", ("fill1025",), 10, 2, 0.9),
                SC.Run("mates", ("mates",), 200, 2, 0.0)]
        self.runs = {r.name: r for r in runs}
        for a in (self.off, self.comps, self.vals):
            a.setflags(write=False)

    def build(self):
        """A fresh host index of the case (not uploaded)."""
        return _native.NativeIndex.build(self.cw, self.dim, self.off, self.comps, self.vals, BuildConfig.defaults(**self.cfg))

    def batch(self, run):
        """(q_off, comps, vals) of a run's queries; `cycle`: the queries repeated in turn up to that many."""
        names = run.queries if not run.cycle else [run.queries[i % len(run.queries)] for i in range(run.cycle)]
        return orc.csr([self.queries[n] for n in names])

    def allowed(self):
        """The filtered calls' allowed documents (a boolean mask): four of five."""
        return np.random.default_rng(77).random(self.n_docs) < 0.8

    def restated(self, run, wrong=None, no_hash=False):
        """(hash_ok, seeds) of a run's batch by the restatement."""
        q_off, qc, _ = self.batch(run)
        return seeds(q_off, qc, self.dim, self.cw, self.value_type, no_hash, wrong)

    def check(self):
        """Asserts on the CPU what every query and batch is there for, and that every wrong reading changes the answer on
        its named case; returns what it found."""
        Q, dim = self.queries, self.dim
        sd = {n: query_seed(c) for n, (c, _) in Q.items()}
        assert [len(Q[n][0]) for n in ("empty", "one", "eight", "fill1024", "fill1025", "fail300")] == [0, 1, 8, 1024, 1025, 300]
        # fill edge: 1024 consecutive ids take seed 0 and fill exactly a quarter of the table; 1025 have no seed BY THE RULE
        # (they would have one without it: the restatement with the limit lifted finds it)
        assert sd["fill1024"] == 0 and len(np.unique(hash_slot(Q["fill1024"][0], hash_mult(0)))) == HASH_SLOTS // 4
        assert sd["fill1025"] == HASH_SEEDS and len(np.unique(hash_slot(Q["fill1025"][0], hash_mult(0)))) == 1025
        assert (sd["empty"], sd["one"], sd["seed1"], sd["c2"], sd["c3"], sd["c5"]) == (0, 0, 1, 2, 3, 5)
        assert 16 <= sd["seed16p"] < HASH_SEEDS and sd["seed16p"] < sd["seedmax"] < HASH_SEEDS
        src = "large" if self.vocab == "wide" else self.vocab
        assert dict(seed16p=sd["seed16p"], seedmax=sd["seedmax"]) == SEED_FOUND[src], (sd["seed16p"], sd["seedmax"])
        assert sd["fail300"] == HASH_SEEDS and sd["mates"] < HASH_SEEDS
        assert len({sd[n] for n in CYCLE_POOL}) == len(CYCLE_POOL) == 7 and HASH_SEEDS not in {sd[n] for n in CYCLE_POOL}
        assert CYCLE % 7 == 0 and CYCLE > 4 * 512 and self.runs["mixed"].cycle % 8 == 0
        # large ids
        assert Q["big16"][0].min() >= 1 << 16 and int(Q["last"][0].max()) == DIMS["large" if self.vocab == "wide" else self.vocab] - 1
        if src == "large":
            assert Q["big20"][0].min() >= 1 << 20 and (Q["big20"][0] >= 0xf00000).sum() >= 5
            assert (self.pool >= 0xf00000).sum() >= 200 and ((np.asarray(self.comps) >> 20) == 15).sum() > 1000
        for n in ("big16", "last", "neg", "odd") + (("big20",) if src == "large" else ()):
            assert sd[n] < HASH_SEEDS, n
        # weights
        v = Q["neg"][1]
        assert (v < 0).sum() >= 10 and (v.view(np.uint32) == 0x80000000).sum() == 1
        # slot-mates and the sentinel, under the multiplier of `mates`
        qc, qv = Q["mates"]
        mult = hash_mult(sd["mates"])
        d_src = DIMS[src]
        sent_slot = int(hash_slot([d_src], mult)[0])
        assert int(hash_slot([self.sent_comp], mult)[0]) == sent_slot and self.sent_comp in qc and self.sent_comp != d_src
        assert float(qv[qc == self.sent_comp][0]) == 2.5
        n_pad = n_diff = 0
        margin = np.inf
        for dc, dv in self.mate_docs:
            mates = [int(c) for c in dc if c not in qc and int(hash_slot([c], mult)[0]) in hash_slot(qc, mult)]
            assert len(mates) >= 1 and set(mates) & set(self.mate_ids.values())
            n_pad += len(dc) % 8 != 0
            right, tol = right_score(qc, qv, dc, dv.astype(np.float64))
            wrong = wrong_score(qc, qv, dc, dv, d_src)
            assert abs(wrong - right) > 8 * tol and f32(wrong) != f32(right), (wrong, right, tol)
            margin = min(margin, abs(wrong - right) / tol)
            n_diff += 1
        assert n_pad >= N_MATES // 3 and n_diff == N_MATES
        # every wrong reading changes the answer on its named case
        bites = {}
        for w, names in (("even_mult", ("odd",)), ("wide_mult", ("seed1",)), ("top_bits", ("eight",)), ("last_seed", ("eight",)),
                         ("strict_limit", ("fill1024",))):
            bites[w] = [n for n in names if query_seed(Q[n][0], w) != sd[n]]
            assert bites[w], w
        assert not np.array_equal(hash_slot(WIDE_IDS, hash_mult(0), "wide_comp"), hash_slot(WIDE_IDS, hash_mult(0)))
        below = np.concatenate([self.pool, self.heads, [(1 << 24) - 1]])
        for s in (0, 1, 63):      # ... and no id below 2^24 can tell: the reason for the dim < 2^24 rule
            assert np.array_equal(hash_slot(below, hash_mult(s), "wide_comp"), hash_slot(below, hash_mult(s)))
        bites["wide_comp"] = ["WIDE_IDS"]
        ok, s_mixed = self.restated(self.runs["mixed"])
        ok_w, s_w = self.restated(self.runs["mixed"], "skip_failed")
        assert (ok, ok_w) == (0, 1) if self.vocab != "wide" else (ok, ok_w) == (0, 0)
        if self.vocab != "wide":
            assert (s_mixed[:7] == [sd[n] for n in CYCLE_POOL]).all() and (s_mixed[7:] == 0).all() and (s_w[8:15] == s_mixed[:7]).all()
            bites["skip_failed"] = ["mixed"]
            assert set(bites) == set(WRONG)
            for name, want in (("sizes", 1), ("cycle", 1), ("mixed", 0), ("alone", 1), ("alone_fit", 1), ("rule", 0), ("mates", 1)):
                assert self.restated(self.runs[name])[0] == want, name
        return dict(seeds=sd, bites=bites, wrong_score_margin_in_bounds=float(margin), padded_mate_documents=int(n_pad),
                    seeded_share_128_160=self.seedmax_share)


@functools.lru_cache(maxsize=None)
def make(vocab):
    """The case of a vocabulary (built once per process; its arrays are read-only)."""
    return HashCase(vocab)


def hook(case, ix, run, env, hash_ok, **over):
    """sgpu_debug_launch_config for a run under an environment, told hash_ok (no device)."""
    Q = case.batch(run)
    with _knobs(env):
        return _native.debug_launch_config(heap_factor=run.hf, **dict(SC.plan_facts(case, ix, run, Q), hash_ok=hash_ok, **over))


def _knobs(env):
    import coop_cases as CC
    return CC.knobs(env)


# the variants of a resident-batch launch: name -> environment (SGPU_BLOCK is added per workgroup size)
VARIANTS = {"loop": dict(SGPU_COOP="0", SGPU_STREAM="0"), "stream": dict(SGPU_COOP="0"), "coop": dict(SGPU_COOP="force")}
BLOCKS = SC.BLOCKS
