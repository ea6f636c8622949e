"""The float64 model of tests/model64.py, proved on the CPU side: the oracle's and the host library's answers stay within
the model's conditions (both summation orders, plain and filtered, both builders), and every checker rejects the damage it
is there to find. No GPU. Lines starting "model64:" report how tight the derived bounds are (run with -s)."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

# (case, value type): every case as binary16, two of the non-negative ones also with fixed-u8 values, one as DotVByte
VARIANTS = [(name, 0) for name in M64.CASES] + [("exp_w2_300", 1), ("exp_w2_300", 2), ("flat_w4_70000", 1)]
VARIANT_IDS = ["%s-vt%d" % v for v in VARIANTS]
ORDERS = [orc.ORDER_LANES16, orc.ORDER_SEQ]


def _continuous(S):
    """Where at least 90 % of the rows must be unambiguous, so that the exact-set assertion carries the weight: every
    law but the three-level one, in every storage (the wide fixed-u8 variant draws from the bounded law for that:
    model64.VALUE_LAWS)."""
    return S["law"] != "ties"
KS_SEARCH = (1, 10, 64, 65, 129, 1000)


def _say(what, **kv):
    print("model64: %-34s %s" % (what, " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v)
                                                 for k, v in kv.items())))


@functools.lru_cache(maxsize=None)
def _host(name):
    cw, dim, D, Q, law, cfg = M64.make_case(name)
    return _native.NativeIndex.build(cw, dim, *D, BuildConfig.defaults(**cfg))


@functools.lru_cache(maxsize=None)
def _setup(name, vt):
    """The oracle's index of a case (converted with the oracle's own restatement for vt 1; DotVByte stores the same
    host arrays, so vt 2 takes the host library's conversion), the model of it and the modelled queries."""
    cw, dim, D, Q, law, cfg = M64.make_case(name)
    keep = orc.OracleIndex(cw, dim, *D, BuildConfig.defaults(**cfg))
    if vt == 1:
        keep = keep.convert_fixedu8()
    elif vt == 2:
        keep = _host(name).convert(2)
    desc = keep.desc
    model = M64.Model(orc.desc_arrays(desc), desc.val_scale, desc.value_type)
    queries = [model.query(*M64.query_at(Q, i), index=i) for i in range(len(Q[0]) - 1)]
    return dict(keep=keep, desc=desc, model=model, queries=queries, Q=Q, law=law, cfg=cfg, D=D, cw=cw, dim=dim)


def _pad(sc, ids, k):
    s, i = np.zeros(k, np.float32), np.zeros(k, np.uint64)
    s[: len(sc)], i[: len(ids)] = sc, ids
    return s, i


def _check_exact_rows(S, rows, k, pool=None, tally=None):
    """rows: (scores [nq, k], ids [nq, k], n [nq]). check_topk's verdicts go to `tally`; returns the worst score ratio."""
    model, worst = S["model"], 0.0
    tally = M64.Tally() if tally is None else tally
    sc, ids, n = rows
    for q in S["queries"]:
        i, m = q.index, int(n[q.index])
        model.check_rows(sc[i], ids[i], m, k, i)
        worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
        tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], pool, k))
    return worst


@pytest.mark.parametrize("order", ORDERS, ids=["lanes16", "seq"])
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_oracle_exact_search_is_the_models_topk(variant, order):
    S = _setup(*variant)
    nq = len(S["queries"])
    tally, worst = M64.Tally(), 0.0
    for k in M64.KS:
        sc, ids, n = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)
        for q in S["queries"]:
            s, i = orc.exact_search(S["desc"], q.comps, q.vals.astype(np.float32), k, order)
            n[q.index] = len(s)
            sc[q.index], ids[q.index] = _pad(s, i, k)
        worst = max(worst, _check_exact_rows(S, (sc, ids, n), k, None, tally))
    _say("oracle exact %s order %d" % ("%s-vt%d" % variant, order), unambiguous=tally, score_ratio=worst)
    assert worst <= 1.0
    if _continuous(S):
        assert tally.share >= 0.9, str(tally)


@pytest.mark.parametrize("order", ORDERS, ids=["lanes16", "seq"])
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_oracle_approximate_search_stays_within_the_model(variant, order):
    S = _setup(*variant)
    model, desc, Q = S["model"], S["desc"], S["Q"]
    nonneg = S["law"] != "signed"
    worst, tally, witnessed = 0.0, M64.Tally(), 0
    # exhaustive: heap_factor 0 on non-negative data skips nothing, the answer is the top-k of C whatever the walk order
    for qcut in (1, 4, 1000) if nonneg else ():
        for k in KS_SEARCH:
            for srt in (False, True):
                sc, ids, n = orc.batch_search(desc, *Q, k, qcut, 0.0, srt, order=order)[:3]
                for q in S["queries"]:
                    i, m = q.index, int(n[q.index])
                    model.check_rows(sc[i], ids[i], m, k, i)
                    worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
                    tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], model.candidates(q, qcut), k))
    for hf in (0.5, 0.8, 1.0, 1.3):
        for qcut in (1, 2, 3, 5, 8, 12):
            k = KS_SEARCH[(qcut + int(hf * 10)) % len(KS_SEARCH)]
            sc, ids, n = orc.batch_search(desc, *Q, k, qcut, hf, bool(qcut % 2), order=order)[:3]
            for q in S["queries"]:
                i, m = q.index, int(n[q.index])
                model.check_rows(sc[i], ids[i], m, k, i)
                worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
                if nonneg:
                    witnessed += model.check_pruned(q, ids[i, :m], sc[i, :m], k, qcut, hf)
                else:
                    assert np.isin(ids[i, :m].astype(np.int64), model.candidates(q, qcut)).all(), i
    _say("oracle search %s order %d" % ("%s-vt%d" % variant, order), unambiguous=tally if nonneg else "n/a",
         score_ratio=worst, skipped_better_documents=witnessed)
    assert worst <= 1.0
    if _continuous(S) and nonneg:
        assert tally.share >= 0.9, str(tally)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_oracle_summary_dots_are_the_models(variant):
    S = _setup(*variant)
    model, worst, n = S["model"], 0.0, 0
    lists = np.flatnonzero(np.diff(model.lbs) > 0)
    for q in S["queries"]:
        for c in list(lists[:: max(1, len(lists) // 6)]) + [int(x) for x in model.selected_lists(q, 2)]:
            got = orc.summary_distances(S["desc"], int(c), q.comps, q.vals.astype(np.float32)).astype(np.float64)
            dot, tol = model.summary_dots(int(c), q)
            assert len(got) == len(dot)
            r = np.where(got == dot, 0.0, np.abs(got - dot) / np.where(tol > 0, tol, 1e-300))
            assert (r <= 1.0).all(), (q.index, c, int(np.argmax(r)), r.max())
            worst, n = max(worst, float(r.max()) if len(r) else 0.0), n + len(r)
    _say("oracle summary dots %s-vt%d" % variant, blocks=n, dot_ratio=worst)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_host_exact_search_plain_and_filtered(variant):
    name, vt = variant
    S = _setup(name, vt)
    ix = _host(name) if vt == 0 else _host(name).convert(vt)
    model = M64.Model(orc.desc_arrays(ix.desc), ix.desc.val_scale, ix.desc.value_type)
    H = dict(S, model=model, queries=[model.query(q.comps, q.vals, index=q.index) for q in S["queries"]])
    rng = np.random.default_rng(5)
    n_docs = model.n_docs
    filters = [None, np.flatnonzero(rng.random(n_docs) < 0.3), rng.choice(n_docs, 70, replace=False),
               np.zeros(0, np.int64)]
    tally, worst = M64.Tally(), 0.0
    for allowed in filters:
        f = None if allowed is None else ix.make_filter(allowed)
        for k in M64.KS:
            got = ix.exact_search(*S["Q"], k, filter=f)
            worst = max(worst, _check_exact_rows(H, got, k, allowed, tally if allowed is None else None))
    _say("host exact %s-vt%d" % variant, unambiguous=tally, score_ratio=worst)
    if _continuous(S):
        assert tally.share >= 0.9, str(tally)


# ---- the built index ----
def _index_arrays(ix):
    d = ix.desc
    return orc.desc_arrays(d), d.val_scale, d.value_type


@pytest.mark.parametrize("name", list(M64.CASES) + ["edges"])
def test_both_builders_build_what_the_header_describes(name):
    if name == "edges":
        cw, dim, D, cfg = M64.edge_inputs()
        v16 = M64.f16_of(D[2]).view(np.uint16)
        # the inputs do reach the branches: subnormal results, values flushed to zero, saturation, ties to even
        assert ((v16 & 0x7c00) == 0).sum() > 20 and (v16 == 0x7bff).sum() > 3 and (v16 == 0xfbff).sum() > 1
        assert (v16 == 0x3c00).sum() >= 1 and (v16 == 0x3c02).sum() >= 1     # 1 + 2^-11 -> 1.0, 1 + 3 * 2^-11 -> 1 + 2^-9
    else:
        cw, dim, D, Q, law, cfg = M64.make_case(name)
    oi = orc.OracleIndex(cw, dim, *D, BuildConfig.defaults(**cfg))
    M64.check_index(orc.desc_arrays(oi.desc), D, cfg)
    ix = _native.NativeIndex.build(cw, dim, *D, BuildConfig.defaults(**cfg))
    M64.check_index(*_index_arrays(ix)[:1], D, cfg)
    if name != "edges":
        for vt, conv in [(1, oi.convert_fixedu8()), (1, ix.convert(1))] + ([(2, ix.convert(2))] if cw == 2 else []):
            a, scale, got_vt = _index_arrays(conv)         # (conv keeps the arrays alive)
            assert got_vt == vt
            M64.check_index(a, D, cfg, scale, vt)


# ---- mutations: every checker can fail ----
ROWS = 50


def _exact_rows(S, k, order=orc.ORDER_LANES16):
    for q in S["queries"]:
        s, i = orc.exact_search(S["desc"], q.comps, q.vals.astype(np.float32), k, order)
        yield q, s, i.astype(np.int64)


def _mutation_cases():
    for variant in VARIANTS:
        yield _setup(*variant)


def test_mutation_one_term_removed_from_one_score():
    done, smallest = 0, np.inf
    rng = np.random.default_rng(1)
    for S in _mutation_cases():
        model = S["model"]
        for q, s, ids in _exact_rows(S, 10):
            for j in np.flatnonzero(q.m[ids] >= 1):
                terms = model.terms(q, int(ids[j]))
                terms = terms[terms != 0]
                if len(terms) == 0:
                    continue
                drop = terms[int(rng.integers(len(terms)))]
                bad = s.copy()
                bad[j] = np.float32(q.s[ids[j]] - drop)
                smallest = min(smallest, float(model.score_ratio(q, ids[j: j + 1], bad[j: j + 1])[0]))
                with pytest.raises(AssertionError, match="document %d " % ids[j]):
                    model.check_scores(q, ids, bad)
                done += 1
    _say("mutation: one term removed", rows=done, smallest_error_over_tol=smallest)
    assert done >= ROWS and smallest > 10.0      # an order of magnitude above 1: the cases' values discriminate


def test_mutation_score_off_by_four_tolerances():
    done = 0
    for S in _mutation_cases():
        model = S["model"]
        for q, s, ids in _exact_rows(S, 10, orc.ORDER_SEQ):
            ok = np.flatnonzero(q.tol[ids] > 0)
            if len(ok) == 0:
                continue
            j = ok[q.index % len(ok)]
            bad = s.astype(np.float64)
            bad[j] = q.s[ids[j]] + 4 * q.tol[ids[j]]
            if abs(np.float32(bad[j]) - q.s[ids[j]]) <= q.tol[ids[j]]:
                continue          # (cannot happen for f32 scores: 4 tol is more than an ulp; kept as a guard)
            with pytest.raises(AssertionError, match="document %d " % ids[j]):
                model.check_scores(q, ids, bad)
            done += 1
    assert done >= ROWS, done


def test_mutation_id_swapped_for_rank_k_plus_5():
    done = 0
    for S in _mutation_cases():
        model = S["model"]
        for k in (10, 64):
            for q, s, ids in _exact_rows(S, k):
                order = np.argsort(-q.s, kind="stable")
                T = q.tol.max()
                if model.n_docs < k + 5 or not q.s[order[k - 1]] - q.s[order[k + 4]] > 4 * T:
                    continue
                bad_i, bad_s = ids.copy(), s.copy()
                bad_i[-1], bad_s[-1] = order[k + 4], np.float32(q.s[order[k + 4]])
                model.check_rows(bad_s, bad_i, k, k)
                model.check_scores(q, bad_i, bad_s)       # the row is well-formed and truthfully scored ...
                with pytest.raises(AssertionError, match="document %d " % order[k + 4]):
                    model.check_topk(q, bad_i, bad_s, None, k)   # ... but it is not the top-k
                done += 1
    assert done >= ROWS, done


def test_mutation_duplicated_id():
    done = 0
    for S in _mutation_cases():
        for q, s, ids in _exact_rows(S, 10):
            bad_i, bad_s = ids.copy(), s.copy()
            j = 1 + q.index % 9
            bad_i[j], bad_s[j] = bad_i[j - 1], bad_s[j - 1]
            with pytest.raises(AssertionError, match="document %d returned more than once" % bad_i[j]):
                S["model"].check_rows(bad_s, bad_i, 10, 10)
            done += 1
    assert done >= ROWS, done


def test_mutation_id_from_outside_the_candidates():
    done = 0
    for S in _mutation_cases():
        if S["law"] == "signed":
            continue
        model = S["model"]
        for hf, checker in ((0.0, "topk"), (0.9, "pruned")):
            sc, ids, n = orc.batch_search(S["desc"], *S["Q"], 10, 2, hf, False)[:3]
            for q in S["queries"]:
                m = int(n[q.index])
                C = model.candidates(q, 2)
                outside = np.setdiff1d(np.arange(model.n_docs), C)
                if m == 0 or len(outside) == 0:
                    continue
                # the best outsider: truthfully scored, and placed where the row stays sorted
                d = outside[np.argmax(q.s[outside])]
                bad_i = ids[q.index, :m].astype(np.int64)
                bad_s = sc[q.index, :m].copy()
                bad_i[-1], bad_s[-1] = d, min(np.float32(q.s[d]), bad_s[-1])
                with pytest.raises(AssertionError, match="document %d " % d):
                    if checker == "topk":
                        model.check_topk(q, bad_i, bad_s, C, 10)
                    else:
                        model.check_pruned(q, bad_i, bad_s, 10, 2, hf)
                done += 1
    assert done >= ROWS, done


def test_mutation_disallowed_id_under_a_filter():
    done = 0
    for variant in VARIANTS:
        name, vt = variant
        S = _setup(name, vt)
        ix = _host(name) if vt == 0 else _host(name).convert(vt)
        model = M64.Model(orc.desc_arrays(ix.desc), ix.desc.val_scale, ix.desc.value_type)
        allowed = np.flatnonzero(np.random.default_rng(6).random(model.n_docs) < 0.5)
        sc, ids, n = ix.exact_search(*S["Q"], 10, filter=ix.make_filter(allowed))
        banned = np.setdiff1d(np.arange(model.n_docs), allowed)
        for q0 in S["queries"]:
            q = model.query(q0.comps, q0.vals, index=q0.index)
            m = int(n[q.index])
            bad_i, bad_s = ids[q.index, :m].astype(np.int64), sc[q.index, :m].copy()
            model.check_topk(q, bad_i, bad_s, allowed, 10)
            d = banned[np.argmax(q.s[banned])]       # a banned document that may well belong to the unfiltered top-k
            bad_i[0], bad_s[0] = d, max(np.float32(q.s[d]), bad_s[0])
            with pytest.raises(AssertionError, match="document %d is outside the pool" % d):
                model.check_topk(q, bad_i, bad_s, allowed, 10)
            done += 1
    assert done >= ROWS, done


@functools.lru_cache(maxsize=None)
def _small_index():
    """A small index for the structural mutations (check_index runs once per mutation)."""
    cw, dim, D, cfg = M64.edge_inputs()
    D = (D[0], D[1], np.abs(np.clip(D[2], -100, 100)) + np.float32(0.01))
    oi = orc.OracleIndex(cw, dim, *D, BuildConfig.defaults(**cfg))
    return oi, D, cfg


def test_mutation_summary_code_changed_by_two():
    oi, D, cfg = _small_index()
    A = {k: v.copy() for k, v in orc.desc_arrays(oi.desc).items()}
    m = M64.check_index(A, D, cfg)
    ent_row = np.repeat(np.arange(len(m.row_comp)), np.diff(m.row_ptr))
    ent_blk = m.lbs[np.repeat(np.arange(m.dim), np.diff(m.lrs))[ent_row]] + m.sum_bid
    usable = np.flatnonzero(m.blk_quant[ent_blk] > 1e-3 * np.abs(m.blk_min[ent_blk]))
    assert len(usable) >= ROWS
    for e in np.random.default_rng(7).choice(usable, ROWS, replace=False):
        was = int(A["sum_code"][e])
        A["sum_code"][e] = was + 2 if (was <= 253 and e % 2) or was < 2 else was - 2
        with pytest.raises(AssertionError, match="block %d " % ent_blk[e]):
            M64.check_index(A, D, cfg)
        A["sum_code"][e] = was
    M64.check_index(A, D, cfg)


def test_mutation_document_moved_to_another_block():
    """Two postings of neighbouring blocks of one list change places and the summaries stay: where the moved document
    alone carried a summarised maximum of its block by more than the quantisation step, the summary no longer
    describes the block."""
    oi, D, cfg = _small_index()
    A = {k: v.copy() for k, v in orc.desc_arrays(oi.desc).items()}
    m = M64.check_index(A, D, cfg)
    v = M64.f16_of(D[2]).astype(np.float64)
    done = 0
    for c in np.flatnonzero(np.diff(m.lbs) >= 2):
        rows = np.arange(m.lrs[c], m.lrs[c + 1])
        for b in range(m.lbs[c], m.lbs[c + 1] - 1):
            p0, p1 = m.bps[b], m.bps[b + 1]
            if p1 - p0 < 2 or done >= ROWS:
                continue
            lb = b - m.lbs[c]
            kept = [int(m.row_comp[r]) for r in rows if lb in m.sum_bid[m.row_ptr[r]: m.row_ptr[r + 1]]]
            docs = m.post_doc[p0:p1]
            vals = {int(d): dict(zip(m.comp[m.off[d]: m.off[d + 1]], v[m.off[d]: m.off[d + 1]])) for d in docs}
            hit = None
            for d in docs:
                for comp in kept:
                    others = max([vals[int(o)].get(comp, -np.inf) for o in docs if o != d])
                    if vals[int(d)].get(comp, -np.inf) - others > 3 * m.blk_quant[b] + 1e-3:
                        hit = int(d)
            other = int(m.post_doc[p1])          # first posting of the next block of the same list
            if hit is None or any(vals[hit].get(comp, -np.inf) <= dict(
                    zip(m.comp[m.off[other]: m.off[other + 1]], v[m.off[other]: m.off[other + 1]])).get(comp, -np.inf)
                    for comp in kept):
                continue
            at = p0 + int(np.flatnonzero(docs == hit)[0])
            A["post_doc"][at], A["post_doc"][p1] = other, hit
            # the summary of the block that lost the document, or of the one that received it, is no longer within a
            # quantisation step of the block's maximum (or names a component no document of the block has any more)
            with pytest.raises(AssertionError, match=r"block (%d|%d) \(list %d\).*(dequantises to|none of its documents has)"
                                                     % (b, b + 1, c)):
                M64.check_index(A, D, cfg)
            A["post_doc"][at], A["post_doc"][p1] = hit, other
            done += 1
    M64.check_index(A, D, cfg)
    assert done >= ROWS, done


def test_mutation_skipped_block():
    """A returned document that is no near-tie is removed, the row shifted up and the freed last slot given to the best
    candidate not in the row: a full, sorted, truthfully scored row that could only come from skipping a block whose
    summary dot is above the threshold."""
    done = 0
    for S in _mutation_cases():
        if S["law"] == "signed":
            continue
        model = S["model"]
        for hf in (0.0, 0.8):
            sc, ids, n = orc.batch_search(S["desc"], *S["Q"], 10, 3, hf, False)[:3]
            for q in S["queries"]:
                if int(n[q.index]) < 10:
                    continue
                row_i, row_s = ids[q.index].astype(np.int64), sc[q.index].copy()
                model.check_pruned(q, row_i, row_s, 10, 3, hf)
                C = model.candidates(q, 3)
                rest = C[~np.isin(C, row_i)]
                if len(rest) == 0:
                    continue
                fill = rest[np.argmax(q.s[rest])]
                fill_s = min(np.float32(q.s[fill]), row_s[-1])
                # the victim: the best-ranked document that clears the new k-th score and sits in a block the model
                # says could not be skipped against that score
                for j in range(9):
                    d = row_i[j]
                    if not q.s[d] > fill_s + 2 * q.tol[d]:
                        break
                    blocked = False
                    for c in model.selected_lists(q, 3):
                        b0, b1 = model.lbs[c], model.lbs[c + 1]
                        posts = model.post_doc[model.bps[b0]: model.bps[b1]]
                        blk = np.repeat(np.arange(b1 - b0), np.diff(model.bps[b0: b1 + 1]))
                        dot, tol_dot = model.summary_dots(int(c), q)
                        for b in blk[posts == d]:
                            blocked |= bool(dot[b] >= 1.01 * (hf * fill_s + tol_dot[b] + hf * q.tol[d]) + 1e-6)
                    if not blocked:
                        continue
                    bad_i = np.r_[row_i[:j], row_i[j + 1:], fill]
                    bad_s = np.r_[row_s[:j], row_s[j + 1:], fill_s].astype(np.float32)
                    model.check_rows(bad_s, bad_i, 10, 10)
                    with pytest.raises(AssertionError, match="document %d .*cannot have been skipped" % d):
                        model.check_pruned(q, bad_i, bad_s, 10, 3, hf)
                    done += 1
                    break
    assert done >= ROWS, done
