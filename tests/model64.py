"""A float64 statement of what the index and the searches MEAN, written from the descriptor's description in
include/seismic_hip.h. TEST INFRASTRUCTURE, pure numpy.

It is a second opinion next to oracle/: it does not restate the sequential algorithm and calls no project code. It
states properties any correct implementation has, with rounding bounds that are derived, not tuned:

  score      s*(q,d) = sum_c q_c * v_{d,c} in float64 (each product is exact: 24 + 11 significant bits);
             an f32 evaluation in ANY order, with or without FMA contraction, is within
             tol(q,d) = gamma(m+1) * A(q,d),  A = sum |q_c v_{d,c}|,  m = matching components,
             gamma(n) = n u / (1 - n u),  u = 2^-24   (Higham, Accuracy and Stability, 3.1; the model's own f64 error is
             below 2^-40 of that and is ignored).
  summary    dot*(b) = sum_j q_j * (code * blk_quant[b] + blk_min[b]) over the matching rows of the list; an f32
             evaluation is within gamma(m+3) * sum_j |q_j| (code * blk_quant[b] + |blk_min[b]|): two roundings in the
             dequantisation, one in the product, m in the additions. (For blk_min >= 0 the magnitude is |q_j * deq|; a
             negative blk_min cancels against code * quant, and the rounding of that product does not shrink with it.)
  candidates C(q, query_cut) = the documents of the posting lists of the query_cut heaviest query components
             (descending weight, ties by ascending component id).

Input: the dict of arrays of tests/orc.py desc_arrays(desc) (ctypes views of a descriptor), val_scale, value_type.
The second half of the file holds the datasets the two model test files share.
"""
import numpy as np

U = 2.0 ** -24
F16_MAX = 65504.0


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _i64(a):
    return np.asarray(a).astype(np.int64)


def _ranges(starts, lens):
    """Concatenated aranges [starts[i], starts[i] + lens[i]) and the index i of every element."""
    starts, lens = _i64(starts), _i64(lens)
    total = int(lens.sum())
    owner = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    if total == 0:
        return np.zeros(0, np.int64), owner
    first = np.cumsum(lens) - lens
    return starts[owner] + (np.arange(total, dtype=np.int64) - first[owner]), owner


def decode_values(fwd_vals, val_scale, value_type):
    """Document values as the header states them: F16 bit patterns, or code * val_scale (FIXEDU8, DOTVBYTE)."""
    if value_type == 0:
        return np.ascontiguousarray(fwd_vals, np.uint16).view(np.float16).astype(np.float64)
    return np.asarray(fwd_vals).astype(np.float64) * float(val_scale)


class Query:
    """One query with its float64 scores against every document."""

    def __init__(self, index, comps, vals, s, a, m, tol):
        self.index, self.comps, self.vals = index, comps, vals
        self.s, self.a, self.m, self.tol = s, a, m, tol


class Tally:
    """check_topk's verdicts over many rows: `share` = unambiguous rows / rows that had a set to choose (the trivial
    rows, whose pool holds no more than k documents, are counted apart and do not enter it)."""

    def __init__(self):
        self.clear = self.chosen = self.trivial = 0

    def add(self, verdict):
        if verdict is None:
            self.trivial += 1
        else:
            self.chosen += 1
            self.clear += bool(verdict)

    @property
    def share(self):
        return self.clear / self.chosen if self.chosen else float("nan")

    def __str__(self):
        return "%.4g (of %d rows; %d trivial rows apart)" % (self.share, self.chosen, self.trivial)


class Model:
    def __init__(self, arrays, val_scale=0.0, value_type=0):
        A = arrays
        self.off = _i64(A["fwd_offsets"])
        self.n_docs = len(self.off) - 1
        self.comp = _i64(A["fwd_comps"])
        self.val = decode_values(A["fwd_vals"], val_scale, value_type)
        self.doc_of = np.repeat(np.arange(self.n_docs, dtype=np.int64), np.diff(self.off))
        self.lbs = _i64(A["list_block_start"])
        self.dim = len(self.lbs) - 1
        self.bps = _i64(A["block_post_start"])
        self.post_doc = _i64(A["post_doc"])
        self.blk_min = np.asarray(A["blk_min"]).astype(np.float64)
        self.blk_quant = np.asarray(A["blk_quant"]).astype(np.float64)
        self.lrs = _i64(A["list_row_start"])
        self.row_comp = _i64(A["row_comp"])
        self.row_ptr = _i64(A["row_ptr"])
        self.sum_bid = _i64(A["sum_bid"])
        self.sum_code = np.asarray(A["sum_code"]).astype(np.float64)

    # ---- scores ----
    def query(self, comps, vals, index=-1):
        comps = _i64(comps)
        vals = np.asarray(vals, np.float32).astype(np.float64)
        w = np.zeros(self.dim, np.float64)
        present = np.zeros(self.dim, bool)
        w[comps] = vals
        present[comps] = True
        p = w[self.comp] * self.val
        s = np.bincount(self.doc_of, p, self.n_docs)
        a = np.bincount(self.doc_of, np.abs(p), self.n_docs)
        m = np.bincount(self.doc_of, present[self.comp], self.n_docs).astype(np.int64)
        return Query(index, comps, vals, s, a, m, gamma(m + 1) * a)

    def scores(self, q):
        return q.s, q.a, q.m

    def terms(self, q, doc):
        """The matching products q_c * v_{d,c} of one document (float64)."""
        lo, hi = self.off[doc], self.off[doc + 1]
        c = self.comp[lo:hi]
        hit = np.isin(c, q.comps)
        w = np.zeros(self.dim, np.float64)
        w[q.comps] = q.vals
        return w[c[hit]] * self.val[lo:hi][hit]

    # ---- lists ----
    def list_postings(self, c):
        return self.post_doc[self.bps[self.lbs[c]]: self.bps[self.lbs[c + 1]]]

    def selected_lists(self, q, query_cut):
        order = np.lexsort((q.comps, -q.vals))        # descending weight, ties by ascending component id
        return q.comps[order[: max(int(query_cut), 0)]]

    def candidates(self, q, query_cut):
        sel = self.selected_lists(q, query_cut)
        if len(sel) == 0:
            return np.zeros(0, np.int64)
        return np.unique(np.concatenate([self.list_postings(int(c)) for c in sel]))

    def work_counts(self, q, query_cut, exhaustive=False):
        """Work counters [0..2] of sgpu_batch_fetch_stats as the header defines them - blocks of the walked lists, summary
        rows matched (rows of those lists whose component the query has), summary entries read (those rows' entries) -
        for any search parameters; with exhaustive=True also [3..6] of a search that may skip nothing (heap_factor 0.0,
        no negative document or query value, no graph: a summary dot is never below 0 * k-th): every block of the walked
        lists passes, [4] = their postings, [5] = the distinct documents among them, [6] = those documents' component
        counts. Which list wins between EQUAL query values is not the header's to say: the values must be distinct."""
        assert len(np.unique(q.vals.astype(np.float32))) == len(q.vals), "query %d: equal values" % q.index
        blocks = rows_n = entries = posts = 0
        for c in self.selected_lists(q, query_cut):
            c = int(c)
            blocks += int(self.lbs[c + 1] - self.lbs[c])
            rows = np.arange(self.lrs[c], self.lrs[c + 1], dtype=np.int64)
            rows = rows[np.isin(self.row_comp[rows], q.comps)]
            rows_n += len(rows)
            entries += int((self.row_ptr[rows + 1] - self.row_ptr[rows]).sum())
            posts += int(self.bps[self.lbs[c + 1]] - self.bps[self.lbs[c]])
        out = [blocks, rows_n, entries]
        if exhaustive:
            assert (self.val >= 0).all() and (q.vals >= 0).all(), "query %d: negative values, blocks may be skipped" % q.index
            pool = self.candidates(q, query_cut)
            out += [blocks, posts, len(pool), int((self.off[pool + 1] - self.off[pool]).sum())]
        return np.array(out, np.int64)

    def summary_dots(self, c, q):
        """(dot*, tolerance) per block of list c, float64."""
        b0, nb = self.lbs[c], self.lbs[c + 1] - self.lbs[c]
        rows = np.arange(self.lrs[c], self.lrs[c + 1], dtype=np.int64)
        rc = self.row_comp[rows]
        hit = np.isin(rc, q.comps)
        rows, rc = rows[hit], rc[hit]
        w = np.zeros(self.dim, np.float64)
        w[q.comps] = q.vals
        e, owner = _ranges(self.row_ptr[rows], self.row_ptr[rows + 1] - self.row_ptr[rows])
        b = self.sum_bid[e]
        assert (b < nb).all(), "summary entry names a block outside list %d" % c
        qv = w[rc][owner]
        cq = self.sum_code[e] * self.blk_quant[b0 + b]
        mn = self.blk_min[b0 + b]
        dot = np.bincount(b, qv * (cq + mn), nb)
        mag = np.bincount(b, np.abs(qv) * (cq + np.abs(mn)), nb)
        m = np.bincount(b, None, nb)
        return dot, gamma(m + 3) * mag

    # ---- checkers ----
    def check_rows(self, scores, ids, n, k, query_index=-1):
        """One result row as the ABI promises it: n <= k, unique ids below n_docs, best first, slots past n untouched."""
        n = int(n)
        assert n <= k, "query %d: n = %d above k = %d" % (query_index, n, k)
        ids, scores = np.asarray(ids), np.asarray(scores)
        got = ids[:n].astype(np.int64)
        bad = got[got >= self.n_docs]
        assert len(bad) == 0, "query %d: document %d is not below n_docs = %d" % (query_index, bad[0], self.n_docs)
        u, cnt = np.unique(got, return_counts=True)
        assert (cnt == 1).all(), "query %d: document %d returned more than once" % (query_index, u[cnt > 1][0])
        down = np.flatnonzero(np.diff(scores[:n].astype(np.float64)) > 0)
        assert len(down) == 0, "query %d: scores rise at rank %d (document %d)" % (
            query_index, down[0] + 1 if len(down) else -1, got[down[0] + 1] if len(down) else -1)
        assert not ids[n:].any() and not scores[n:].view(np.uint32).any(), \
            "query %d: slots at or beyond n = %d were written" % (query_index, n)

    def score_ratio(self, q, ids, scores):
        """|returned - s*| / tol per returned document (0 where both vanish)."""
        ids = _i64(ids)
        err = np.abs(np.asarray(scores).astype(np.float64) - q.s[ids])
        tol = q.tol[ids]
        return np.where(err == 0, 0.0, err / np.where(tol > 0, tol, np.finfo(np.float64).tiny))

    def check_scores(self, q, ids, scores):
        """Every returned score is the FULL query's dot product with that document, within tol(q, d)."""
        r = self.score_ratio(q, ids, scores)
        bad = np.flatnonzero(r > 1.0)
        if len(bad):
            d = int(_i64(ids)[bad[0]])
            raise AssertionError("query %d: document %d scored %.9g, model %.17g +- %.3g (%.1f x tol)" % (
                q.index, d, float(np.asarray(scores)[bad[0]]), q.s[d], q.tol[d], r[bad[0]]))
        return float(r.max()) if len(r) else 0.0

    def check_topk(self, q, ids, scores, pool, k):
        """The band rule for `ids` = the top-k of `pool` (None = every document). Returns True where the row was
        unambiguous (the set was compared exactly with the model's), False where only the band rule could speak, None
        where the pool holds no more than k documents (everything is returned: there was no set to choose)."""
        ids = _i64(ids)
        pool = np.arange(self.n_docs, dtype=np.int64) if pool is None else np.unique(_i64(pool))
        want_n = min(int(k), len(pool))
        assert len(ids) == want_n, "query %d: %d results, the pool of %d allows %d (document -1)" % (
            q.index, len(ids), len(pool), want_n)
        out = ids[~np.isin(ids, pool)]
        assert len(out) == 0, "query %d: document %d is outside the pool" % (q.index, out[0] if len(out) else -1)
        if len(pool) <= k:
            return None                      # everything is returned (ids are unique: check_rows)
        s = q.s[pool]
        T = float(q.tol[pool].max())
        order = np.argsort(-s, kind="stable")
        t, nxt = s[order[k - 1]], s[order[k]]
        must = pool[s > t + 2 * T]
        miss = must[~np.isin(must, ids)]
        assert len(miss) == 0, "query %d: document %d (s* = %.17g) is above the k-th %.17g by more than 2T = %.3g " \
            "and is missing" % (q.index, miss[0] if len(miss) else -1, q.s[miss[0]] if len(miss) else 0, t, 2 * T)
        low = ids[q.s[ids] < t - 2 * T]
        assert len(low) == 0, "query %d: document %d (s* = %.17g) is below the k-th %.17g by more than 2T = %.3g " \
            "and was returned" % (q.index, low[0] if len(low) else -1, q.s[low[0]] if len(low) else 0, t, 2 * T)
        unambiguous = bool(t - nxt > 2 * T)
        if unambiguous:
            want = np.sort(pool[order[:k]])
            diff = np.setxor1d(want, ids)
            assert len(diff) == 0, "query %d: unambiguous row, document %d differs from the model's set" % (
                q.index, diff[0] if len(diff) else -1)
        return unambiguous

    def check_pruned(self, q, ids, scores, k, query_cut, heap_factor):
        """Necessary condition of the skip rule `heap full && dot < heap_factor * kth` (heap_factor >= 0, no graph):
        the k-th score only rises, so a candidate that clearly beats the final k-th and is missing was never scored,
        hence EVERY block holding it was skipped, against a threshold no higher than the final one."""
        assert heap_factor >= 0
        ids = _i64(ids)
        sel = self.selected_lists(q, query_cut)
        C = self.candidates(q, query_cut)
        out = ids[~np.isin(ids, C)]
        assert len(out) == 0, "query %d: document %d is in none of the %d selected lists" % (
            q.index, out[0] if len(out) else -1, len(sel))
        if len(ids) < k:
            self.check_topk(q, ids, scores, C, k)      # the heap never filled: nothing may have been skipped
            return 0
        t_f = float(np.asarray(scores)[k - 1])
        rest = C[~np.isin(C, ids)]
        off = rest[q.s[rest] > t_f + 2 * q.tol[rest]]
        if len(off) == 0:
            return 0
        for c in sel:
            c = int(c)
            b0, b1 = self.lbs[c], self.lbs[c + 1]
            posts = self.post_doc[self.bps[b0]: self.bps[b1]]
            blk = np.repeat(np.arange(b1 - b0, dtype=np.int64), np.diff(self.bps[b0: b1 + 1]))
            at = np.flatnonzero(np.isin(posts, off))
            if len(at) == 0:
                continue
            dot, tol_dot = self.summary_dots(c, q)
            b, d = blk[at], posts[at]
            bound = heap_factor * t_f + tol_dot[b] + heap_factor * q.tol[d]
            bad = np.flatnonzero(~(dot[b] < bound))
            if len(bad):
                i = bad[0]
                raise AssertionError(
                    "query %d: document %d (s* = %.9g > k-th %.9g) is missing, but block %d of list %d has summary "
                    "dot %.9g >= heap_factor * k-th = %.9g: it cannot have been skipped" % (
                        q.index, d[i], q.s[d[i]], t_f, b[i], c, dot[b[i]], heap_factor * t_f))
        return len(off)


# ---------------------------------------------------------------------------------------------------------------------
# The structure of a built index, independent of both builders.
# ---------------------------------------------------------------------------------------------------------------------
def f16_of(vals):
    """What the forward index stores for finite f32 input: saturate, then round to nearest even (numpy's cast)."""
    return np.clip(np.asarray(vals, np.float32), -F16_MAX, F16_MAX).astype(np.float16)


def fixedu8_of(v16):
    """The header's FIXEDU8 rule on the binary16 values: val_scale = the smallest power of two, from 2^-8 (Q0.8) up,
    with 255 * val_scale >= the largest value; code = min(255, round_half_away(v / val_scale)), negatives -> 0."""
    v = np.asarray(v16).astype(np.float64)
    vmax = max(float(v.max()) if len(v) else 0.0, 0.0)
    scale = 2.0 ** -8
    while 255.0 * scale < vmax:
        scale *= 2.0
    code = np.minimum(255.0, np.floor(np.maximum(v, 0.0) / scale + 0.5))
    return scale, code.astype(np.uint8)


def _cfg(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def check_index(arrays, inputs, cfg, val_scale=0.0, value_type=0):
    """arrays: desc_arrays of the index; inputs = (offsets, comps, f32 values) it was built from; cfg: n_postings,
    max_fraction, summary_energy (a dict or a BuildConfig)."""
    A = arrays
    off, comps, vals = inputs
    off, comps = _i64(off), _i64(comps)
    n_docs = len(off) - 1
    v16 = f16_of(vals)
    m = Model(A, val_scale, value_type)
    dim = m.dim

    # ---- forward index ----
    assert np.array_equal(m.off, off), "fwd_offsets differ from the input (document -1)"
    assert np.array_equal(m.comp, comps), "fwd_comps differ from the input (document -1)"
    doc_of = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(off))
    if value_type == 0:
        bad = np.flatnonzero(np.asarray(A["fwd_vals"]).view(np.uint16) != v16.view(np.uint16))
        assert len(bad) == 0, "document %d: stored binary16 0x%04x, input %r rounds to 0x%04x" % (
            doc_of[bad[0]], A["fwd_vals"][bad[0]], vals[bad[0]], v16.view(np.uint16)[bad[0]])
    else:
        scale, code = fixedu8_of(v16)
        assert float(val_scale) == scale, "val_scale %r, the header's rule gives %r (document -1)" % (val_scale, scale)
        bad = np.flatnonzero(np.asarray(A["fwd_vals"]) != code)
        assert len(bad) == 0, "document %d: stored code %d, the header's rule gives %d" % (
            doc_of[bad[0]], A["fwd_vals"][bad[0]], code[bad[0]])
    v = v16.astype(np.float64)                      # lists and summaries are built on the binary16 values

    # ---- lists and blocks ----
    n_blocks, n_post = len(m.bps) - 1, len(m.post_doc)
    assert m.lbs[0] == 0 and m.lbs[-1] == n_blocks and (np.diff(m.lbs) >= 0).all(), "list_block_start (document -1)"
    assert m.bps[0] == 0 and m.bps[-1] == n_post, "the blocks do not cover the postings (document -1)"
    empty = np.flatnonzero(np.diff(m.bps) <= 0)
    assert len(empty) == 0, "block %d is empty or overlaps its neighbour (document -1)" % (empty[0] if len(empty) else -1)
    blk_list = np.repeat(np.arange(dim, dtype=np.int64), np.diff(m.lbs))
    post_blk = np.repeat(np.arange(n_blocks, dtype=np.int64), np.diff(m.bps))
    post_list = blk_list[post_blk]
    assert (m.post_doc < n_docs).all(), "a posting names a document >= n_docs"
    pkey = post_list * n_docs + m.post_doc
    u, cnt = np.unique(pkey, return_counts=True)
    assert (cnt == 1).all(), "list %d holds document %d more than once" % (
        (u[cnt > 1][0] // n_docs, u[cnt > 1][0] % n_docs) if (cnt > 1).any() else (-1, -1))
    fkey = doc_of * dim + comps                     # ascending: documents in order, components ascending within one
    assert (np.diff(fkey) > 0).all(), "input components are not ascending within a document"
    want = m.post_doc * dim + post_list
    pos = np.searchsorted(fkey, want)
    ok = (pos < len(fkey)) & (fkey[np.minimum(pos, len(fkey) - 1)] == want) if len(fkey) else np.zeros(len(want), bool)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, "list %d holds document %d, which does not have that component" % (
        (post_list[bad[0]], m.post_doc[bad[0]]) if len(bad) else (-1, -1))
    post_val = v[pos]

    # ---- pruning ----
    n_postings = int(_cfg(cfg, "n_postings"))
    cap = int(np.float32(n_postings) * np.float32(_cfg(cfg, "max_fraction")))
    tot = dim * n_postings
    V = -np.inf if len(v) <= tot else np.sort(v)[len(v) - tot]
    bad = np.flatnonzero(post_val < V)
    assert len(bad) == 0, "list %d keeps document %d with value %r below the global threshold %r" % (
        (post_list[bad[0]], m.post_doc[bad[0]], post_val[bad[0]], V) if len(bad) else (-1, -1, 0, 0))
    list_len = np.bincount(post_list, None, dim)
    assert (list_len <= cap).all(), "list %d is longer than the cap %d (document -1)" % (int(np.argmax(list_len)), cap)
    list_min = np.full(dim, np.inf)
    np.minimum.at(list_min, post_list, post_val)
    kept = np.zeros(len(fkey), bool)
    kept[pos] = True
    gone = np.flatnonzero(~kept & (v > V))
    bad = gone[(list_len[comps[gone]] < cap) | (list_min[comps[gone]] < v[gone])]
    assert len(bad) == 0, "document %d is missing from list %d: value %r is above the threshold %r, the list has %d of " \
        "%d postings, its smallest value is %r" % ((doc_of[bad[0]], comps[bad[0]], v[bad[0]], V, list_len[comps[bad[0]]],
                                                    cap, list_min[comps[bad[0]]]) if len(bad) else (-1,) * 7)

    # ---- summaries ----
    # M_b: component-wise maximum over the block's documents, for every (block, component) at once
    e, owner = _ranges(off[m.post_doc], off[m.post_doc + 1] - off[m.post_doc])
    key = post_blk[owner] * dim + comps[e]
    order = np.argsort(key, kind="stable")
    key, ev = key[order], v[e][order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, np.int64)
    mkey = key[first]
    M = np.maximum.reduceat(ev, first) if len(first) else np.zeros(0)
    mblk = mkey // dim

    n_rows = len(m.row_comp)
    assert m.lrs[0] == 0 and m.lrs[-1] == n_rows and (np.diff(m.lrs) >= 0).all(), "list_row_start (document -1)"
    assert m.row_ptr[0] == 0 and m.row_ptr[-1] == len(m.sum_bid) and (np.diff(m.row_ptr) > 0).all(), \
        "row_ptr: a summary row is empty or the rows do not cover the entries (document -1)"
    row_list = np.repeat(np.arange(dim, dtype=np.int64), np.diff(m.lrs))
    same = row_list[1:] == row_list[:-1]
    assert (np.diff(m.row_comp)[same] > 0).all(), "row_comp is not ascending within a list (document -1)"
    ent_row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(m.row_ptr))
    ent_list = row_list[ent_row]
    bad = np.flatnonzero(m.sum_bid >= (m.lbs[ent_list + 1] - m.lbs[ent_list]))
    assert len(bad) == 0, "a summary entry of list %d names block %d, which the list does not have (document -1)" % (
        (ent_list[bad[0]], m.sum_bid[bad[0]]) if len(bad) else (-1, -1))
    inrow = ent_row[1:] == ent_row[:-1]
    assert (np.diff(m.sum_bid)[inrow] > 0).all(), "sum_bid is not ascending within a row (document -1)"
    ent_blk = m.lbs[ent_list] + m.sum_bid
    skey = ent_blk * dim + m.row_comp[ent_row]
    sp = np.searchsorted(mkey, skey)
    ok = (sp < len(mkey)) & (mkey[np.minimum(sp, max(len(mkey) - 1, 0))] == skey) if len(mkey) else np.zeros(len(skey), bool)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, "block %d (list %d) summarises component %d, which none of its documents has (document -1)" % (
        (ent_blk[bad[0]], ent_list[bad[0]], m.row_comp[ent_row[bad[0]]]) if len(bad) else (-1, -1, -1))
    sM = M[sp]
    deq = m.sum_code * m.blk_quant[ent_blk] + m.blk_min[ent_blk]
    ulp = np.spacing(np.maximum(np.abs(sM), np.abs(deq)).astype(np.float32)).astype(np.float64)
    bad = np.flatnonzero(np.abs(deq - sM) > m.blk_quant[ent_blk] + 2 * ulp)
    assert len(bad) == 0, "block %d (list %d), component %d: code %d dequantises to %r, the block's maximum is %r, " \
        "quant %r (document -1)" % ((ent_blk[bad[0]], ent_list[bad[0]], m.row_comp[ent_row[bad[0]]], m.sum_code[bad[0]],
                                     deq[bad[0]], sM[bad[0]], m.blk_quant[ent_blk[bad[0]]]) if len(bad) else (-1,) * 7)

    kept_m = np.zeros(len(mkey), bool)
    kept_m[sp] = True
    assert kept_m.sum() == len(skey), "a (block, component) pair is summarised twice (document -1)"
    bfirst = np.flatnonzero(np.r_[True, mblk[1:] != mblk[:-1]])
    assert len(bfirst) == n_blocks, "blocks without components (document -1)"
    kmin = np.minimum.reduceat(np.where(kept_m, M, np.inf), bfirst)
    kmax = np.maximum.reduceat(np.where(kept_m, M, -np.inf), bfirst)
    dmax = np.maximum.reduceat(np.where(kept_m, -np.inf, M), bfirst)
    nkept = np.add.reduceat(kept_m.astype(np.int64), bfirst)
    nall = np.add.reduceat(np.ones(len(M), np.int64), bfirst)
    bad = np.flatnonzero(nkept == 0)
    assert len(bad) == 0, "block %d has no summary (document -1)" % (bad[0] if len(bad) else -1)
    bad = np.flatnonzero(m.blk_min != kmin)
    assert len(bad) == 0, "block %d: blk_min %r, the smallest kept maximum is %r (document -1)" % (
        (bad[0], m.blk_min[bad[0]], kmin[bad[0]]) if len(bad) else (-1, 0, 0))
    wantq = (kmax - kmin) / 255.0
    bad = np.flatnonzero(np.abs(m.blk_quant - wantq) > 2 * np.spacing(wantq.astype(np.float32)).astype(np.float64))
    assert len(bad) == 0, "block %d: blk_quant %r, (max - min) / 255 is %r (document -1)" % (
        (bad[0], m.blk_quant[bad[0]], wantq[bad[0]]) if len(bad) else (-1, 0, 0))
    # energy: the kept components are the largest ones, the first prefix of them (by descending value) whose mass
    # reaches summary_energy * total. Stated so that it also holds where values are negative: either everything is
    # kept or the mass reaches the target; without the smallest kept one it would not.
    bad = np.flatnonzero(kmin < dmax)
    assert len(bad) == 0, "block %d keeps a component of %r and drops one of %r (document -1)" % (
        (bad[0], kmin[bad[0]], dmax[bad[0]]) if len(bad) else (-1, 0, 0))
    energy = float(np.float32(_cfg(cfg, "summary_energy")))
    mass = np.add.reduceat(np.where(kept_m, M, 0.0), bfirst)
    total = np.add.reduceat(M, bfirst)
    slack = gamma(nall) * np.add.reduceat(np.abs(M), bfirst)
    bad = np.flatnonzero((nkept < nall) & (mass < energy * total - slack))
    assert len(bad) == 0, "block %d keeps mass %r of %r: below summary_energy = %r (document -1)" % (
        (bad[0], mass[bad[0]], total[bad[0]], energy) if len(bad) else (-1, 0, 0, 0))
    bad = np.flatnonzero((nkept > 1) & ~(mass - kmin < energy * total + slack))
    assert len(bad) == 0, "block %d keeps mass %r of %r: more components than summary_energy = %r needs (document -1)" % (
        (bad[0], mass[bad[0]], total[bad[0]], energy) if len(bad) else (-1, 0, 0, 0))
    return m


# ---------------------------------------------------------------------------------------------------------------------
# Datasets shared by test_model_cpu.py (oracle and host results) and test_gpu_model.py (device results).
# ---------------------------------------------------------------------------------------------------------------------
VALUE_LAWS = {
    "exp": lambda rng, n: (rng.exponential(0.5, n) + 0.01).astype(np.float32),
    "ties": lambda rng, n: rng.choice([0.5, 1.0, 2.0], n).astype(np.float32),
    "signed": lambda rng, n: rng.normal(0, 1, n).astype(np.float32),
    # bounded, for fixed-u8 storage at a wide vocabulary: val_scale follows the LARGEST value, so the exp law's tail leaves
    # its typical value some 16 codes and documents that meet a query in one component tie (0.88 of the rows unambiguous
    # at dim 70 000, whatever the seed); a law without a tail keeps 250 codes (0.93)
    "flat": lambda rng, n: rng.uniform(0.01, 0.99, n).astype(np.float32),
}
KS = (1, 10, 63, 64, 65, 128, 129, 1000)


def _components(rng, n, dim):
    """n distinct components below dim - 1, low ids far more popular, the more so the larger dim (lists of very different
    lengths, many empty ones - the last component's always; most queries meet a good part of the documents)."""
    n = min(n, dim - 1)
    c = np.unique(((dim - 1) * rng.random(3 * n + 8) ** (2 + 1.5 * np.log10(dim))).astype(np.int64))
    if len(c) < n:
        c = np.unique(np.concatenate([c, rng.choice(dim - 1, n, replace=False)]))
    return np.sort(rng.choice(c, n, replace=False)).astype(np.uint32)


def _csr(vecs):
    off = np.zeros(len(vecs) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c, _ in vecs])
    comps = np.concatenate([c for c, _ in vecs] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    vals = np.concatenate([v for _, v in vecs] + [np.zeros(0, np.float32)]).astype(np.float32)
    return off, comps, vals


# name: (component width, dim, documents, law, seed, build configuration)
CASES = {
    "exp_w2_300": (2, 300, 2500, "exp", 11,
                   dict(n_postings=400, centroid_fraction=0.1, summary_energy=0.5, max_fraction=1.5, min_cluster_size=2, doc_cut=15)),
    "signed_w2_3000": (2, 3000, 4000, "signed", 12,
                       dict(n_postings=60, centroid_fraction=0.3, summary_energy=0.9, max_fraction=6.0, min_cluster_size=0, doc_cut=5)),
    "ties_w2_300": (2, 300, 2500, "ties", 13,
                    dict(n_postings=200, centroid_fraction=0.1, summary_energy=0.4, max_fraction=1.0, min_cluster_size=3, doc_cut=15)),
    "exp_w4_70000": (4, 70000, 900, "exp", 14,
                     dict(n_postings=20, centroid_fraction=0.2, summary_energy=1.0, max_fraction=1.5, min_cluster_size=1, doc_cut=10)),
}
# the wide case again for its fixed-u8 variant only (not run as binary16)
CASES_U8 = {
    "flat_w4_70000": (4, 70000, 900, "flat", 14, CASES["exp_w4_70000"][5]),
}


def law_of(name):
    return (CASES.get(name) or CASES_U8[name])[3]


def make_case(name, n_queries=40):
    """(component width, dim, documents CSR, queries CSR, law, build configuration dict). 2 % of the documents are
    empty; two have more than 128 and more than 256 components (where dim allows); query 0 is empty, query 1 has one
    component whose posting list is empty, the others draw 12 to 40 components by the documents' popularity law."""
    cw, dim, n_docs, law, seed, cfg = CASES.get(name) or CASES_U8[name]
    rng = np.random.default_rng(seed)
    values = VALUE_LAWS[law]
    docs = []
    for d in range(n_docs):
        if rng.random() < 0.02:
            docs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        n = int(rng.integers(1, 60))
        if d in (5, 6):
            n = (140, 280)[d - 5]
        c = _components(rng, n, dim)
        docs.append((c, values(rng, len(c))))
    D = _csr(docs)
    lens = np.diff(D[0].astype(np.int64))
    assert (lens == 0).any() and ((lens > 128) & (lens <= 256)).any() and (lens > 256).any(), \
        "case %s: no empty document, or none of more than 128 / more than 256 components" % name
    used = np.zeros(dim, bool)
    used[D[1]] = True
    unused = np.flatnonzero(~used)
    assert len(unused), "case %s: every component is used, no query can meet an empty list" % name
    qs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32)),
          (unused[-1:].astype(np.uint32), np.ones(1, np.float32))]
    while len(qs) < n_queries:
        c = _components(rng, int(rng.integers(12, 41)), dim)
        qs.append((c, values(rng, len(c))))
    return cw, dim, D, _csr(qs), law, dict(cfg)


# where binary16 conversion branches (edge_inputs; the `edges` law of tests/build_cases.py)
EDGE_SPECIAL = np.array([2.0 ** -14, 2.0 ** -15, 3.0e-6, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1e-9,
                         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20,
                         2048 + 1, 2048 + 3, 65504.0, 65519.9, 65520.0, 70000.0, 3.0e38, 0.0,
                         -2.0 ** -25, -1 - 2.0 ** -11, -65520.0, -70000.0, -3.0e-6], np.float32)


def edge_inputs():
    """A small collection whose values sit where binary16 conversion branches: below the normal range, exactly on
    rounding ties (to even, both ways), at and beyond the largest finite value, zero, both signs."""
    rng = np.random.default_rng(15)
    dim, n_docs = 120, 700
    special = EDGE_SPECIAL
    docs = []
    for d in range(n_docs):
        c = _components(rng, int(rng.integers(1, 25)), dim)
        v = VALUE_LAWS["exp"](rng, len(c))
        hit = rng.random(len(c)) < 0.08
        v[hit] = rng.choice(special, int(hit.sum()))
        docs.append((c, v))
    cfg = dict(n_postings=40, centroid_fraction=0.15, summary_energy=0.6, max_fraction=1.5, min_cluster_size=2, doc_cut=8)
    return 2, dim, _csr(docs), cfg


def distinct_weights(Q):
    """The queries of Q with pairwise distinct values inside every query (rank * 2^-13 added, asserted): the inputs of
    the work-count comparisons, where a tie between equal query values would make the walked lists a [CHOICE]."""
    off, c, v = Q
    v = np.asarray(v, np.float32).copy()
    for i in range(len(off) - 1):
        lo, hi = int(off[i]), int(off[i + 1])
        v[lo:hi] += np.arange(hi - lo, dtype=np.float32) * np.float32(2.0 ** -13)
        assert len(np.unique(v[lo:hi])) == hi - lo, "query %d still has equal values" % i
    return off, c, v


def query_at(Q, i):
    off, c, v = Q
    return c[int(off[i]): int(off[i + 1])], v[int(off[i]): int(off[i + 1])]
