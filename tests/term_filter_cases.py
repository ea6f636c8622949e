"""Seeded inputs and the reference for the tests of term filters (test_term_filter_cpu.py, test_gpu_term_filter.py).
TEST INFRASTRUCTURE, pure numpy apart from the index build.

expected_bits() restates, from the text of include/seismic_hip.h alone and over the forward arrays of get_desc(), the set of
sgpu_filter_create_terms[_host]: a clause matches document d iff d stores the component with a decoded value (binary16 ->
f32; u8 code * val_scale) >= min_weight; A = every MUST matches, no MUST_NOT matches, at least min_should SHOULD clauses
match, intersected with `within`. It has one switch per wrong reading (WRONG).

Index shapes (make(n_docs, variant)): n_docs in N_DOCS - the word edge (31, 32, 33), the range edge of 32768 documents
(32767, 32768, 32769: a last range of one document) and three ranges (65541); every seventh document is empty (n_docs == 1:
the one document is not). Components:
  0, 1, 2     stored by about 1/2, 1/3 and 1/10 of the documents
  3           stored only in the last range
  4 ... 11    L_COMP[L]: stored by exactly min(L, what fits) documents, all of one range (the fullest, the later one on a
              tie), for L in LS = 0, 1, 63, 64, 65 and 4095, 4096, 4097 - one below, at and one above the 4096 entries a
              workgroup of term_filter_kernel reads per step (1024 threads x 4)
  dim - 1     stored by about 1/5 (u32 variants: dim = 70000, so the component does not fit u16)
Values come from PALETTE, all exact in binary16: negatives, -0.0, a subnormal and (f16 variants) 65504. The u8 and DotVByte
variants are conversions of the same documents with 2.5 in place of 65504 (the quantisation step follows the largest
value; with 65504 every other code would be 0).
"""
import functools

import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

MUST, MUST_NOT, SHOULD = 0, 1, 2
RANGE = 32768
STEP = 4096                    # entries a workgroup reads per step (kTermBS * kTermE)
N_DOCS = (1, 31, 32, 33, 32767, 32768, 32769, 65541)
VARIANTS = ("u16_f16", "u16_u8", "u16_dvb", "u32_f16", "u32_u8")
LS = (0, 1, 63, 64, 65, STEP - 1, STEP, STEP + 1)
L_COMP = {L: 4 + i for i, L in enumerate(LS)}
LAST_RANGE_COMP = 3
SUBNORMAL = np.float32(2.0 ** -24)
PALETTE = np.array([0.5, 1.0, 1.5, 0.25, 2.0, -1.0, -0.5, -0.0, SUBNORMAL, 65504.0, 0.75, 3.0, 0.0], np.float32)
NINF = float("-inf")


def dim_of(variant):
    return 70000 if variant.startswith("u32") else 40


def _documents(n_docs, dim, big):
    """CSR (off u64, comps u32, vals f32) of the shape the module text describes."""
    rng = np.random.default_rng(4200 + n_docs)
    d = np.arange(n_docs)
    nonempty = (d % 7 != 3) | (n_docs == 1)
    n_ranges = -(-n_docs // RANGE)
    sizes = [min(RANGE, n_docs - r * RANGE) for r in range(n_ranges)]
    full = max(range(n_ranges), key=lambda r: (sizes[r], r))
    cols = sorted([0, 1, 2, LAST_RANGE_COMP] + list(L_COMP.values()) + [dim - 1])
    has = np.zeros((n_docs, len(cols)), bool)
    col = {c: i for i, c in enumerate(cols)}
    for c, p in ((0, 0.5), (1, 1 / 3), (2, 0.1), (dim - 1, 0.2)):
        has[:, col[c]] = rng.random(n_docs) < p
    has[:, col[LAST_RANGE_COMP]] = (d >= (n_ranges - 1) * RANGE) & (rng.random(n_docs) < 0.5)
    in_full = np.flatnonzero(nonempty & (d // RANGE == full))
    for L, c in L_COMP.items():
        has[rng.permutation(in_full)[:L], col[c]] = True
    has[0, col[0]] = True                      # document 0 stores component 0 (a threshold is taken from it)
    has[n_docs - 1, col[LAST_RANGE_COMP]] = True
    has[~nonempty] = False
    rows, cc = np.nonzero(has)                 # row-major: components ascending within a document
    off = np.zeros(n_docs + 1, np.uint64)
    off[1:] = np.cumsum(has.sum(1))
    comps = np.asarray(cols, np.uint32)[cc]
    vals = PALETTE[rng.integers(0, len(PALETTE), len(rows))].copy()
    if not big:
        vals[vals == 65504.0] = 2.5
    if len(vals):
        vals[0] = 1.5                          # the first entry of document 0: component 0 with a value both encodings hold
    return off, comps, vals


class TermIndex:
    def __init__(self, n_docs, variant):
        self.n_docs, self.variant, self.dim = n_docs, variant, dim_of(variant)
        cw = 4 if variant.startswith("u32") else 2
        f16 = variant.endswith("f16")
        self.off, self.comps, self.vals = _documents(n_docs, self.dim, big=f16)
        base = _native.NativeIndex.build(cw, self.dim, self.off, self.comps, self.vals,
                                         BuildConfig.defaults(n_postings=16, centroid_fraction=0.1, summary_energy=0.4))
        self.ix = base if f16 else base.convert(2 if variant.endswith("dvb") else 1)
        self.fwd = forward(self.ix.desc)
        self.n_ranges = -(-n_docs // RANGE)


@functools.lru_cache(maxsize=None)
def make(n_docs, variant):
    """The index of (n_docs, variant), built once per process and not uploaded (upload a .ix of your own copy: fresh())."""
    return TermIndex(n_docs, variant)


def fresh(n_docs, variant):
    """A new index of the same documents (for the tests that upload)."""
    return TermIndex(n_docs, variant)


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def forward(desc):
    """The forward arrays of a descriptor, copied, with the entries also grouped by component."""
    a = orc.desc_arrays(desc)
    off = np.array(a["fwd_offsets"], np.int64)
    comps = np.array(a["fwd_comps"]).astype(np.int64)
    raw = np.array(a["fwd_vals"])
    n_docs = int(desc.n_docs)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(off))
    order = np.argsort(comps, kind="stable")
    return dict(n_docs=n_docs, dim=int(desc.dim), f16=int(desc.value_type) == 0, val_scale=np.float32(desc.val_scale), off=off,
                comps=comps, raw=raw, doc=doc, order=order, sorted_comps=comps[order])


def decoded(fwd, raw):
    if fwd["f16"]:
        return raw.view(np.float16).astype(np.float32)
    return raw.astype(np.float32) * fwd["val_scale"]


WRONG = ("gt", "u8_code", "f16_bits", "should_distinct", "min_should_0_as_1", "must_not_ignored_without_must",
         "complement_past_end", "last_range_dropped", "within_or")


def expected_bits(fwd, clauses, min_should, within=None, wrong=None):
    """The words of the set (u32, ceil(n_docs / 32), at least one). clauses: (component, occur, min_weight) triples;
    within: bool [n_docs] or None. wrong: None, or one of WRONG -
      gt                              the comparison is > instead of >=
      u8_code                         the threshold is compared against the u8 code, not code * val_scale
      f16_bits                        binary16 values and the threshold (rounded to binary16) are compared as bit patterns
      should_distinct                 SHOULD matches are counted per distinct component, not per clause
      min_should_0_as_1               min_should == 0 is read as 1
      must_not_ignored_without_must   MUST_NOT clauses are dropped when there is no MUST clause
      complement_past_end             the bits of the last word at and past n_docs are treated as empty documents
      last_range_dropped              the documents of the last range of 32768 are left out
      within_or                       `within` is OR-ed in instead of AND-ed"""
    assert wrong is None or wrong in WRONG
    n_docs = fwd["n_docs"]
    n_words = max(-(-n_docs // 32), 1)
    must = np.zeros(n_docs, np.int64)
    should = np.zeros(n_docs, np.int64)
    banned = np.zeros(n_docs, bool)
    n_must = sum(1 for _, o, _ in clauses if o == MUST)
    seen_should = {}
    for c, occur, mw in clauses:
        lo, hi = np.searchsorted(fwd["sorted_comps"], [c, c + 1])
        ent = fwd["order"][lo:hi]
        raw = fwd["raw"][ent]
        mw = np.float32(mw)
        if wrong == "u8_code" and not fwd["f16"]:
            v = raw.astype(np.float32)
        elif wrong == "f16_bits" and fwd["f16"]:
            v, mw = raw.astype(np.int64), int(np.float32(mw).astype(np.float16).view(np.uint16))
        else:
            v = decoded(fwd, raw)
        hit = fwd["doc"][ent[(v > mw) if wrong == "gt" else (v >= mw)]]
        if occur == MUST:
            must[hit] += 1
        elif occur == MUST_NOT:
            banned[hit] = True
        elif wrong == "should_distinct":
            m = seen_should.setdefault(c, np.zeros(n_docs, bool))
            m[hit] = True
        else:
            should[hit] += 1
    if wrong == "should_distinct":
        for m in seen_should.values():
            should += m
    if wrong == "must_not_ignored_without_must" and n_must == 0:
        banned[:] = False
    need = 1 if (wrong == "min_should_0_as_1" and min_should == 0) else min_should
    ok = (must == n_must) & ~banned & (should >= need)
    if wrong == "last_range_dropped":
        ok[(-(-n_docs // RANGE) - 1) * RANGE:] = False
    if within is not None:
        ok = (ok | within) if wrong == "within_or" else (ok & within)
    padded = np.zeros(n_words * 32, bool)
    padded[:n_docs] = ok
    if wrong == "complement_past_end" and n_must == 0 and need == 0 and within is None:
        padded[n_docs:] = True
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def bits_diff(got, want):
    """None where the words are equal, else a sentence naming the first differing word."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape/dtype %s %s != %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    i = int(bad[0])
    return "word %d (documents %d..%d, range %d): got %08x, want %08x; %d words differ" % (
        i, 32 * i, 32 * i + 31, 32 * i // RANGE, int(got[i]), int(want[i]), len(bad))


# ---------------------------------------------------------------------------------------------------------------------
# clause sets and `within` sets
# ---------------------------------------------------------------------------------------------------------------------
def clause_sets(t):
    """name -> (clauses, min_should) for the index t (a TermIndex)."""
    dim, fwd = t.dim, t.fwd
    v0 = float(decoded(fwd, fwd["raw"][:1])[0]) if len(fwd["raw"]) else 1.0   # document 0's value of component 0
    above = float(np.nextafter(np.float32(v0), np.float32(np.inf)))
    three = [(0, SHOULD, NINF), (1, SHOULD, NINF), (2, SHOULD, 0.5)]
    out = {
        "none": ([], 0),
        "must_frequent": ([(0, MUST, NINF)], 0),
        "must_two": ([(0, MUST, NINF), (1, MUST, 0.5)], 0),
        "must_not": ([(0, MUST_NOT, NINF)], 0),
        "must_not_weight": ([(1, MUST_NOT, 1.0), (2, MUST_NOT, NINF)], 0),
        "should_twice": ([(0, SHOULD, 0.5), (0, SHOULD, 1.5)], 2),
        "should_twice_one": ([(0, SHOULD, 0.5), (0, SHOULD, 1.5)], 1),
        "at_value": ([(0, MUST, v0)], 0),
        "above_value": ([(0, MUST, above)], 0),
        "plus_zero": ([(1, MUST, 0.0)], 0),          # a stored -0.0 matches
        "minus_zero": ([(1, MUST, -0.0)], 0),
        "subnormal": ([(1, MUST, float(SUBNORMAL))], 0),
        "negative": ([(1, MUST, -0.75)], 0),
        "huge": ([(0, SHOULD, 65504.0), (1, SHOULD, 65504.0)], 1),
        "last_range": ([(LAST_RANGE_COMP, MUST, NINF)], 0),
        "last_component": ([(dim - 1, MUST, NINF)], 0),
        "mixed": ([(0, MUST, NINF), (2, MUST_NOT, NINF), (1, SHOULD, 0.5), (dim - 1, SHOULD, NINF)], 1),
        "must_not_and_should0": ([(2, MUST_NOT, NINF), (1, SHOULD, NINF)], 0),
    }
    for ms in (0, 1, 3, 4):
        out["should3_min%d" % ms] = (three, ms)
    for L, c in L_COMP.items():
        out["L%d" % L] = ([(c, MUST, NINF)], 0)
        out["notL%d" % L] = ([(c, MUST_NOT, NINF)], 0)
    # 1024 clauses: 1000 SHOULD over every used component with thresholds from the palette, 20 repeats of one MUST, four MUST_NOT
    rng = np.random.default_rng(77)
    used = [0, 1, 2, LAST_RANGE_COMP] + list(L_COMP.values()) + [dim - 1]
    many = [(int(rng.choice(used[:3] + [dim - 1])), SHOULD, float(PALETTE[rng.integers(0, len(PALETTE))])) for _ in range(1000)]
    many += [(0, MUST, NINF)] * 20 + [(L_COMP[65], MUST_NOT, NINF), (2, MUST_NOT, 2.0), (L_COMP[STEP], MUST_NOT, 0.5),
                                       (1, MUST_NOT, 65504.0)]
    order = rng.permutation(len(many))
    out["c1024"] = ([many[i] for i in order], 150)
    out["c1024_all_should"] = ([many[i] for i in order], 1001)
    return out


def within_sets(n_docs):
    """name -> bool [n_docs]"""
    d = np.arange(n_docs)
    sparse = d % 97 == 5
    sparse[[0, min(31, n_docs - 1), min(32, n_docs - 1), n_docs - 1]] = True
    return {"sparse": sparse, "empty": np.zeros(n_docs, bool), "full": np.ones(n_docs, bool)}


WITHIN_CLAUSES = ("none", "must_frequent", "must_not", "mixed")

# the case on which each wrong reading differs from the contract: (n_docs, variant, clause set, within or None)
WRONG_CASES = {
    "gt": (33, "u16_f16", "at_value", None),
    "u8_code": (33, "u16_u8", "at_value", None),
    "f16_bits": (33, "u16_f16", "negative", None),
    "should_distinct": (33, "u16_f16", "should_twice", None),
    "min_should_0_as_1": (33, "u16_f16", "should3_min0", None),
    "must_not_ignored_without_must": (33, "u16_f16", "must_not", None),
    "complement_past_end": (33, "u16_f16", "must_not", None),
    "last_range_dropped": (32769, "u16_f16", "last_range", None),
    "within_or": (33, "u16_f16", "must_frequent", "sparse"),
}
