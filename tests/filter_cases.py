"""Seeded inputs and the reference for the tests of a filter's device view (test_filter_cases_cpu.py,
test_gpu_filter_view.py). TEST INFRASTRUCTURE, pure numpy apart from the index build.

The view (seismic_amd/csrc/filter.hip) is the replica's block_post_start, post_ref and post_doc with the postings of
documents outside the allowed set A deleted, and the kNN graph with the neighbours outside A replaced by 0xffffffff.
expected_view() says that with plain array operations. The cases put posting counts and kept-posting patterns on the edges
of the kernels that build the view: flag words of 64 postings, tiles of 2048, a scan in passes of 4096 tiles, a block remap
with one arm for starts at a multiple of 64 and one for a start at n_postings.

  exact_<P>   P documents of one component each over five lists (and a few empty documents), built so that pruning keeps
              every entry: n_postings == P for P = 0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 5000
  blocks      16 lists of small clusters, 2560 postings: block starts at and off multiples of 64, the last start at
              n_postings = 40 whole words, lists that the holes set empties
  big         8 400 037 postings, 4102 tiles: the scan's second pass with a carry (GPU only apart from its check())

In these three every posting belongs to a document of its own (posting p <-> document post_doc[p]), so that an allowed set
can be aimed at posting positions: allowed_sets() derives them from post_doc of the built index and says, for each, the
kept-posting mask it is meant to give; check_sets() asserts it.

The second half restates the device algorithm in numpy (device_view) with one switch per wrong reading;
test_filter_cases_cpu.py shows that each disagrees with expected_view on a named small case.
"""
import functools

import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

WORD = 64                 # postings per flag word (one ballot)
TILE = 32 * WORD          # kTile
PASS_TILES = 4 * 1024     # tile counts per pass of filter_scan_kernel
NONE = np.uint32(0xffffffff)

EXACT_COUNTS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 5000)
EXACT_DIM = 5
BIG_P = 8_400_037
BIG_DIM = 64


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def bitmap(allowed):
    """ceil(n_docs / 32) words (at least one), bit d of word d / 32, the bits past n_docs zero."""
    n_words = max((len(allowed) + 31) // 32, 1)
    padded = np.zeros(n_words * 32, bool)
    padded[:len(allowed)] = allowed
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def expected_view(base, allowed, n_docs):
    """The view of the allowed set (bool [n_docs]) on the replica whose arrays are `base`."""
    allowed = np.asarray(allowed, bool)
    assert len(allowed) == n_docs
    post_doc = np.asarray(base["post_doc"], np.uint32)
    keep = allowed[post_doc]
    before = np.zeros(len(post_doc) + 1, np.int64)          # kept postings before position p
    np.cumsum(keep, dtype=np.int64, out=before[1:])
    knn = np.asarray(base["knn"], np.uint32)
    inside = knn < n_docs
    inside[inside] = allowed[knn[inside]]
    return dict(block_post_start=before[np.asarray(base["block_post_start"]).astype(np.int64)].astype(np.uint32),
                post_ref=np.asarray(base["post_ref"], np.uint64)[keep], post_doc=post_doc[keep],
                knn=np.where(inside, knn, NONE).astype(np.uint32), bits=bitmap(allowed), count=int(allowed.sum()))


VIEW_ARRAYS = ("block_post_start", "post_ref", "post_doc", "knn", "bits")


def view_diff(got, want):
    """None where the two views are equal; otherwise a sentence naming the first differing array, the first differing
    index, its tile, word and lane, and the two values."""
    for k in VIEW_ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != w.dtype:
            return "%s: dtype %s != %s" % (k, g.dtype, w.dtype)
        n = min(len(g), len(w))
        bad = np.flatnonzero(g[:n] != w[:n])
        if len(bad) or len(g) != len(w):
            i = int(bad[0]) if len(bad) else n
            return "%s[%d] (tile %d, word %d, lane %d): got %s, want %s; lengths %d, %d; %d of the common elements differ" % (
                k, i, i // TILE, i // WORD, i % WORD, hex(int(g[i])) if i < len(g) else "nothing",
                hex(int(w[i])) if i < len(w) else "nothing", len(g), len(w), len(bad))
    if got["count"] != want["count"]:
        return "count: got %d, want %d" % (got["count"], want["count"])
    return None


def host_base(desc, knn=None):
    """The arrays of an unfiltered replica as far as a host descriptor knows them: block_post_start and post_doc are the
    descriptor's, post_ref is made up (distinct 64-bit words with both halves in use), knn is `knn` or empty."""
    a = orc.desc_arrays(desc)
    p = np.arange(int(desc.n_postings), dtype=np.uint64)
    return dict(block_post_start=a["block_post_start"].astype(np.uint32), post_doc=np.array(a["post_doc"], np.uint32),
                post_ref=(p * np.uint64(0x9e3779b97f4a7c15)) | np.uint64(1),
                knn=np.zeros(0, np.uint32) if knn is None else np.asarray(knn, np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class FilterCase:
    def __init__(self, name, cw, dim, off, comps, vals, cfg, check, paths, single=True):
        self.name, self.cw, self.dim = name, cw, dim
        self.off, self.comps, self.vals = off, comps, np.asarray(vals, np.float32)
        self.n_docs = len(off) - 1
        self.cfg, self._check, self.paths = cfg, check, paths
        self.single = single           # every posting belongs to a document of its own
        for a in (self.off, self.comps, self.vals):
            a.setflags(write=False)

    def build(self, use_device=0):
        """A fresh index of the case (not uploaded). use_device: BuildConfig.use_device (device + 1; the same index)."""
        return _native.NativeIndex.build(self.cw, self.dim, self.off, self.comps, self.vals,
                                         BuildConfig.defaults(use_device=use_device, **self.cfg))

    def check(self, desc):
        """Asserts the case's properties from the descriptor of an index built from it; returns what it found."""
        a = orc.desc_arrays(desc)
        assert int(desc.n_docs) == self.n_docs
        if self.single:
            assert len(np.unique(a["post_doc"])) == int(desc.n_postings)
        return self._check(self, desc, a)


def _single_component(rng, n_docs, holders, dim, signed):
    """CSR of n_docs documents of which `holders` (ascending ids) carry one component each, the others none."""
    off = np.zeros(n_docs + 1, np.uint64)
    has = np.zeros(n_docs, np.int64)
    has[holders] = 1
    off[1:] = np.cumsum(has)
    comps = rng.integers(0, dim, len(holders)).astype(np.uint32)
    vals = (rng.exponential(0.45, len(holders)) + 0.02).astype(np.float32)
    if signed:
        vals[rng.random(len(holders)) < 0.3] *= -1.0
    return off, comps, vals


def _exact(P):
    rng = np.random.default_rng(700 + P)
    # P holders and an empty document after every sixteenth one; at least 45 documents (ids 0, 31, 32 and the last exist
    # and the last bitmap word is partial)
    n_docs = max(P + P // 16, 45)
    if n_docs % 32 == 0:
        n_docs += 3
    ids = np.arange(n_docs)
    holders = ids[ids % 17 != 16][:P] if P else ids[:0]
    if len(holders) < P:
        holders = ids[:P]
    off, comps, vals = _single_component(rng, n_docs, holders, EXACT_DIM, signed=True)
    cfg = dict(n_postings=max(P, 1), centroid_fraction=0.1, min_cluster_size=2, summary_energy=0.4, max_fraction=1.0)
    return FilterCase("exact_%d" % P, 2, EXACT_DIM, off, comps, vals, cfg, _check_exact,
                      "n_postings = %d: %d flag word(s), the last holding %d; %d tile(s)" % (
                          P, -(-P // WORD), P - (P - 1) // WORD * WORD if P else 0, -(-P // TILE)))


def _check_exact(case, desc, a):
    P = int(case.name[6:])
    assert int(desc.n_postings) == P == int(case.off[-1]) and len(a["post_doc"]) == P
    bps = a["block_post_start"].astype(np.int64)
    assert len(bps) == int(desc.n_blocks) + 1 and bps[0] == 0 and bps[-1] == P and (np.diff(bps) >= 0).all()
    assert case.n_docs >= 45 and case.n_docs % 32 != 0
    if P == 0:
        assert not np.diff(case.off.astype(np.int64)).any()          # all documents empty
    return dict(n_postings=P, n_blocks=int(desc.n_blocks), words=-(-P // WORD), tiles=-(-P // TILE), n_docs=case.n_docs)


BLOCKS_LISTS, BLOCKS_TAGS, BLOCKS_NP = 16, 16, 80
BLOCKS_P = (BLOCKS_LISTS + BLOCKS_TAGS) * BLOCKS_NP        # 2560 = 40 words


def _blocks(seed=811):
    """Every document: a list component c < 16 with a positive value and a tag component 16 + t with the value -8. Documents
    of a list gather around the sampled centroids that share their tag (8 x 8 outweighs the list component), so a list
    falls into clusters of a few to a few dozen documents; pruning keeps the dim x n_postings = 2560 largest entries, which
    are exactly the positive ones: the tag lists stay empty and every posting belongs to a document of its own."""
    rng = np.random.default_rng(seed)
    n_docs = BLOCKS_P + 9                                    # nine empty documents at the end
    c = rng.integers(0, BLOCKS_LISTS, BLOCKS_P)
    t = BLOCKS_LISTS + rng.integers(0, BLOCKS_TAGS, BLOCKS_P)
    v = (rng.exponential(0.45, BLOCKS_P) + 0.02).astype(np.float32)
    off = np.zeros(n_docs + 1, np.uint64)
    off[1:BLOCKS_P + 1] = 2 * np.arange(1, BLOCKS_P + 1)
    off[BLOCKS_P + 1:] = 2 * BLOCKS_P
    comps = np.stack([c, t], 1).reshape(-1).astype(np.uint32)
    vals = np.stack([v, np.full(BLOCKS_P, -8.0, np.float32)], 1).reshape(-1)
    cfg = dict(n_postings=BLOCKS_NP, centroid_fraction=0.1, min_cluster_size=2, summary_energy=0.4, max_fraction=4.0)
    return FilterCase("blocks", 2, BLOCKS_LISTS + BLOCKS_TAGS, off, comps, vals, cfg, _check_blocks,
                      "block starts at and off multiples of 64 (the r == 0 arm), the last start at n_postings = 40 words (the "
                      "total arm), lists and first blocks the holes set empties")


def _check_blocks(case, desc, a):
    P = int(desc.n_postings)
    bps, lbs = a["block_post_start"].astype(np.int64), a["list_block_start"].astype(np.int64)
    assert P == BLOCKS_P and P % WORD == 0 and bps[-1] == P                  # the last start takes the total arm
    inner = bps[(bps > 0) & (bps < P)]
    at, off = inner[inner % WORD == 0], inner[inner % WORD != 0]
    assert len(at) >= 1 and len(off) >= 1, (at, off)
    sizes = np.diff(bps)
    assert int(desc.n_blocks) >= 5 * BLOCKS_LISTS and np.median(sizes) <= 24
    assert (np.diff(lbs)[:BLOCKS_LISTS] >= 3).all() and not np.diff(lbs)[BLOCKS_LISTS:].any()   # the tag lists are empty
    # the holes set empties a whole list that has postings, and a first block
    holes = holes_set(desc, case.n_docs)
    keep = holes[a["post_doc"]]
    emptied = [c for c in range(case.dim) if bps[lbs[c + 1]] > bps[lbs[c]] and not keep[bps[lbs[c]]:bps[lbs[c + 1]]].any()]
    assert len(emptied) >= 1 and keep.any()
    return dict(n_blocks=int(desc.n_blocks), starts_at_a_word=at.tolist(), starts_inside_a_word=len(off),
                lists_emptied_by_holes=emptied, largest_block=int(sizes.max()))


def _big():
    """8 400 037 documents of one component each over 64 lists (document d: component d % 64), one centroid per list
    (centroid_fraction x 131 251 < 1): 64 blocks, a posting per document, the lists' documents ascending."""
    n = BIG_P
    off = np.arange(n + 1, dtype=np.uint64)
    comps = (np.arange(n, dtype=np.uint32) % BIG_DIM).astype(np.uint32)
    vals = (0.05 + (np.arange(n, dtype=np.uint32) % 977).astype(np.float32) / 512.0).astype(np.float32)
    cfg = dict(n_postings=n // BIG_DIM + 1, centroid_fraction=1e-6, min_cluster_size=0, summary_energy=0.4, max_fraction=1.0)
    return FilterCase("big", 2, BIG_DIM, off, comps, vals, cfg, _check_big,
                      "n_postings = 8 400 037: 4102 tiles, the scan's second pass of 6 tiles with a carry")


def _check_big(case, desc, a):
    P = int(desc.n_postings)
    assert P == BIG_P and P > PASS_TILES * TILE + TILE and P % WORD != 0
    assert -(-P // TILE) >= PASS_TILES + 2
    return dict(n_postings=P, tiles=-(-P // TILE), n_blocks=int(desc.n_blocks))


def check_big_sets(sets, post_doc):
    """Kept postings exist in tiles on both sides of tile 4096 (the pass boundary) for every set that keeps any."""
    first_of_pass2 = PASS_TILES * TILE
    out = {}
    for name, (allowed, _) in sets.items():
        keep = allowed[post_doc]
        lo, hi = int(keep[:first_of_pass2].sum()), int(keep[first_of_pass2:].sum())
        if name not in ("none", "first", "last"):
            assert lo > 0 and hi > 0, (name, lo, hi)
        out[name] = (lo, hi)
    return out


CASE_NAMES = tuple("exact_%d" % P for P in EXACT_COUNTS) + ("blocks",)       # (the small ones: "big" is made on request)


@functools.lru_cache(maxsize=None)
def make(name):
    """The case `name` (built once per process; its arrays are read-only)."""
    if name.startswith("exact_"):
        return _exact(int(name[6:]))
    if name == "blocks":
        return _blocks()
    if name == "big":
        return _big()
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# allowed sets
# ---------------------------------------------------------------------------------------------------------------------
def holes_set(desc, n_docs):
    """The holes set of test_gpu_filter._sets: every 7th list emptied, and the first block of every 11th."""
    import test_gpu_filter
    return test_gpu_filter._sets(desc, n_docs, 1)["holes"]


def allowed_sets(desc, post_doc, seed=0, names=None):
    """name -> (allowed bool [n_docs], the kept-posting mask it is meant to give or None), derived from `post_doc` of the
    built index so that the sets hit posting positions. With a posting per document the mask is met exactly; elsewhere a
    document's other postings are kept too (check_sets(..., single=False) asserts the intended ones are among them)."""
    n_docs, P = int(desc.n_docs), len(post_doc)
    rng = np.random.default_rng(900 + seed)
    p = np.arange(P)
    out = {}

    def at(name, mask):
        allowed = np.zeros(n_docs, bool)
        allowed[post_doc[mask]] = True
        out[name] = (allowed, mask)

    out["all"] = (np.ones(n_docs, bool), np.ones(P, bool))
    out["none"] = (np.zeros(n_docs, bool), np.zeros(P, bool))
    if P:
        at("first", p == 0)
        at("last", p == P - 1)
        at("lane0", p % WORD == 0)
        at("lane63", p % WORD == WORD - 1)
        at("lanes31_32", (p % WORD == 31) | (p % WORD == 32))
        at("words_even", (p // WORD) % 2 == 0)
        at("tiles_even", (p // TILE) % 2 == 0)          # kept, dropped, kept ...: empty tiles between full ones
        at("tiles_odd", (p // TILE) % 2 == 1)           # dropped, kept ...
        mid = (P // TILE // 2) * TILE + TILE // 2 - 24  # a posting in the middle of a tile (of the only, partial one: of it)
        at("all_but_one", p != (mid if mid < P else P // 2))
    out["p1"] = (rng.random(n_docs) < 0.01, None)
    out["p50"] = (rng.random(n_docs) < 0.5, None)
    out["holes"] = (holes_set(desc, n_docs), None)
    edge = np.zeros(n_docs, bool)
    edge[[0, 31, 32, n_docs - 1]] = True                # first and last bit of a bitmap word, the last document
    out["doc_ids"] = (edge, None)
    return out if names is None else {k: out[k] for k in names if k in out}


def check_sets(sets, post_doc, single=True):
    found = {}
    for name, (allowed, want) in sets.items():
        keep = allowed[post_doc]
        if want is not None:
            assert np.array_equal(keep, want) if single else keep[want].all(), name
        found[name] = int(keep.sum())
    return found


BIG_SETS = ("all", "first", "last", "lane63", "words_even", "tiles_even", "tiles_odd", "all_but_one", "p1", "p50")


# ---------------------------------------------------------------------------------------------------------------------
# The device algorithm restated in numpy, with one switch per wrong reading.
# ---------------------------------------------------------------------------------------------------------------------
WRONG = ("no_carry", "past_end", "no_r0_arm", "total_is_last_base", "rank_le", "knn_oob")


def device_view(base, allowed, n_docs, pass_tiles=PASS_TILES, wrong=None):
    """filter.hip's view build: a ballot word per 64 postings and a count per tile of 2048 (flag), an exclusive scan of the
    tile counts in passes of `pass_tiles` with a carry (scan), every kept posting to tile base + kept postings of the
    words before it in the tile + kept lanes below it in its word (scatter), every block start p to the base of word p / 64
    + the kept lanes below p % 64 - nothing for p % 64 == 0, the total for p / 64 past the last word (blocks), and the kNN
    mask. Counts are 32-bit. wrong: None, or one of WRONG -
      no_carry            the scan forgets what the passes before held
      past_end            the lanes of the last word at and past n_postings count as kept
      no_r0_arm           a block start at a multiple of 64 takes the full-word mask
      total_is_last_base  a block start at n_postings = 64 n_words takes the last word's base
      rank_le             the rank within a word counts the lanes at or below, not below
      knn_oob             a neighbour id >= n_docs passes the mask"""
    assert wrong is None or wrong in WRONG
    allowed = np.asarray(allowed, bool)
    post_doc, post_ref = np.asarray(base["post_doc"], np.uint32), np.asarray(base["post_ref"], np.uint64)
    bps = np.asarray(base["block_post_start"]).astype(np.int64)
    knn = np.asarray(base["knn"], np.uint32)
    inside = knn < n_docs
    ok = inside.copy()
    ok[inside] = allowed[knn[inside]]
    if wrong == "knn_oob":
        ok |= ~inside
    out = dict(knn=np.where(ok, knn, NONE).astype(np.uint32), bits=bitmap(allowed), count=int(allowed.sum()))
    n_p = len(post_doc)
    if n_p == 0:
        out.update(block_post_start=np.zeros(len(bps), np.uint32), post_ref=post_ref[:0], post_doc=post_doc[:0])
        return out
    n_words, n_tiles = -(-n_p // WORD), -(-n_p // TILE)
    # flag
    lanes = np.zeros(n_tiles * TILE, bool)
    lanes[:n_p] = allowed[post_doc]
    if wrong == "past_end":
        lanes[n_p:n_words * WORD] = True
    src_ref, src_doc = np.zeros(len(lanes), np.uint64), np.zeros(len(lanes), np.uint32)   # (what lies past the end: zeros)
    src_ref[:n_p], src_doc[:n_p] = post_ref, post_doc
    by_word = lanes.reshape(-1, WORD)
    tile_cnt = lanes.reshape(n_tiles, TILE).sum(1).astype(np.int64)
    # scan
    tile_base = np.zeros(n_tiles + 1, np.int64)
    carry = 0
    for b0 in range(0, n_tiles, pass_tiles):
        c = tile_cnt[b0:b0 + pass_tiles]
        start = 0 if wrong == "no_carry" else carry
        tile_base[b0:b0 + len(c)] = start + np.cumsum(c) - c
        carry = start + int(c.sum())
    total = tile_base[n_tiles] = carry
    # scatter
    word_cnt = by_word.sum(1).astype(np.int64)
    in_tile = word_cnt.reshape(n_tiles, TILE // WORD)
    word_base = (tile_base[:n_tiles, None] + np.cumsum(in_tile, 1) - in_tile).reshape(-1)
    upto = np.cumsum(by_word, 1, dtype=np.int64)                 # kept lanes at or below the lane
    rank = upto if wrong == "rank_le" else upto - by_word
    pos = (word_base[:, None] + rank)[by_word]
    size = int(max(total, pos.max() + 1 if len(pos) else 0))
    ref, doc = np.zeros(size, np.uint64), np.zeros(size, np.uint32)
    ref[pos], doc[pos] = src_ref[lanes], src_doc[lanes]
    # blocks
    below = np.concatenate([np.zeros((len(by_word), 1), np.int64), upto], 1)   # [w, r]: kept lanes below lane r of word w
    wi, r = bps >> 6, bps & 63
    if wrong == "no_r0_arm":
        r = np.where(r == 0, WORD, r)
    past = wi >= n_words
    wi_in = np.where(past, n_words - 1, wi)
    start = np.where(past, word_base[n_words - 1] if wrong == "total_is_last_base" else total,
                     word_base[wi_in] + below[wi_in, np.where(past, 0, r)])
    out.update(block_post_start=(start & 0xffffffff).astype(np.uint32), post_ref=ref[:total], post_doc=doc[:total])
    return out
