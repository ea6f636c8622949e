"""The reference side of tests/test_gpu_stage01_edges.py, without a device: every case of tests/stage01_cases.py reaches the
edges it exists for (check()), the oracle's summary dots agree with the float64 model within the model's own tolerance, the
oracle's rows of every run pass the model's checkers, the numpy restatement of the kernel's walk (stage01_cases.walk_dots:
row table, split, chunk prefix, owner search, float32 additions in that order) equals orc.summary_distances bit for bit on
the cases rows, chunks and pairs, and every wrong reading of that restatement is caught by a named case - the cases
discriminate. Lines starting "model64:" report the model's verdicts (run with -s)."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
import stage01_cases as S
import stream_cases as SC


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, host index) - nothing is uploaded."""
    case = S.make(name)
    return case, case.build()


@functools.lru_cache(maxsize=None)
def arrays(name):
    case, ix = built(name)
    a = orc.desc_arrays(ix.desc)
    return a, S.mids(a)


@functools.lru_cache(maxsize=None)
def oracle_dots(name):
    """The oracle's summary dots of every (list, query) pair of a case, in the order of case.dots."""
    case, ix = built(name)
    return tuple(orc.summary_distances(ix.desc, case.P(lst), *case.queries[q]) for lst, q in case.dots)


@functools.lru_cache(maxsize=None)
def oracle_counts(name, run_name):
    """(scores, ids, n, counts) of a run's DISTINCT queries, each on its own."""
    case, ix = built(name)
    run = case.runs[run_name]
    Q = orc.csr([case.queries[n] for n in run.queries])
    return orc.batch_search_counts(ix.desc, *Q, run.k, run.cut, run.hf, run.first_sorted)


@functools.lru_cache(maxsize=None)
def _model(name):
    case, ix = built(name)
    d = ix.desc
    model = M64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    return model, {n: model.query(c, v, index=i) for i, (n, (c, v)) in enumerate(case.queries.items())}


@functools.lru_cache(maxsize=None)
def check_rows_against_the_model(name, run_name):
    """model64's checkers on the oracle's rows of a run (test_gpu_stage01_edges.py calls this once the device's rows are
    these bit for bit): rows well-formed, scores within the model's bound, ids from the walked lists, the top-k of that pool
    where nothing may be skipped, pruning within what the summary dots allow. Returns (tally, worst score ratio)."""
    case, _ = built(name)
    run = case.runs[run_name]
    model, queries = _model(name)
    sc, ids, n, _ = oracle_counts(name, run_name)
    tally, worst = M64.Tally(), 0.0
    for i, qn in enumerate(run.queries):
        q, m = queries[qn], int(n[i])
        model.check_rows(sc[i], ids[i], m, run.k, i)
        worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
        pool = model.candidates(q, run.cut)
        assert np.isin(ids[i, :m].astype(np.int64), pool).all(), (run_name, qn)
        nonneg = len(q.vals) == 0 or q.vals.min() >= 0
        if nonneg and run.hf == 0.0:
            tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], pool, run.k))
        elif nonneg and run.hf > 0 and len(np.unique(q.vals)) == len(q.vals):
            model.check_pruned(q, ids[i, :m], sc[i, :m], run.k, run.cut, run.hf)
    return tally, worst


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_case_reaches_its_edges(name):
    case, ix = built(name)
    assert ix.desc.n_docs == case.n_docs <= 5000 and ix.desc.value_type == case.value_type and ix.desc.comp_width == case.cw
    assert ix.desc.dim == case.dim and (case.cw == 2 or case.comps.min() > 65535)
    print("stage01 case %s: %s" % (name, case.check(ix)))


@pytest.mark.parametrize("name", S.DOT_CASES)
def test_oracle_dots_agree_with_the_model(name):
    case, _ = built(name)
    model, queries = _model(name)
    worst = 0.0
    for (lst, q), got in zip(case.dots, oracle_dots(name)):
        dot, tol = model.summary_dots(case.P(lst), queries[q])
        assert len(got) == len(dot), (lst, q)
        err = np.abs(got.astype(np.float64) - dot)
        assert (err <= tol).all(), (lst, q, int(np.argmax(err - tol)))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()) if len(err) else 0.0)
    print("model64: %-34s summary dots, worst error / tolerance %.4g" % (name, worst))


@pytest.mark.parametrize("name", S.SEARCH_CASES)
def test_oracle_rows_pass_the_models_checkers(name):
    case, _ = built(name)
    total, worst = M64.Tally(), 0.0
    for run_name in case.runs:
        tally, w = check_rows_against_the_model(name, run_name)
        total.clear, total.chosen, total.trivial = total.clear + tally.clear, total.chosen + tally.chosen, total.trivial + tally.trivial
        worst = max(worst, w)
    print("model64: %-34s unambiguous=%s score_ratio=%.4g" % ("oracle stage01 %s" % name, total, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", S.WALK_CASES)
def test_the_restated_walk_equals_the_oracle_bit_for_bit(name):
    case, _ = built(name)
    a, mid = arrays(name)
    for (lst, q), want in zip(case.dots, oracle_dots(name)):
        got = S.walk_dots(a, mid, case.P(lst), *case.queries[q])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lst, q, np.flatnonzero(got != want)[:8])


def _dots_differ(name, **wrong):
    """Some (list, query) of the case whose restated dots under the wrong reading differ from the oracle's."""
    case, _ = built(name)
    a, mid = arrays(name)
    return [(lst, q) for (lst, q), want in zip(case.dots, oracle_dots(name))
            if not np.array_equal(S.walk_dots(a, mid, case.P(lst), *case.queries[q], **wrong).view(np.uint32), want.view(np.uint32))]


def _split_differs(name):
    """The odd list's split points under nb / 2 differ from the directory's (sgpu_debug_row_dir: what the device reads)."""
    from util import row_dir_lookup, row_dir_table
    case, ix = built(name)
    a, mid = arrays(name)
    tab, nbk = row_dir_table(ix)
    lrs = a["list_row_start"].astype(np.int64)
    out = []
    for lst, wrong in ((0, False), (1, True)):                 # the even list splits alike under both readings
        c = case.P(lst)
        rows = np.arange(lrs[c], lrs[c + 1])
        have = np.array([int(row_dir_lookup(tab, nbk, (c << 16) | int(a["row_comp"][r]))[0][3]) & 0xffff for r in rows])
        assert np.array_equal(have, mid[rows])
        assert (not np.array_equal(have, S.mids(a, "down")[rows])) == wrong
        out.append(lst)
    return out[1:]


def _ties_differ(name):
    case, _ = built(name)
    return [q for q in ("tie", "tie_rev") for cut in (1, 3, 5) if S.walked(case, q, cut) != S.walked(case, q, cut, ties="descending")]


def _groups_differ(name):
    case, ix = built(name)
    out = []
    for r in case.runs.values():
        h = S.hook(case, ix, r, 512)
        if S.plan_groups(S.G_NB[: r.cut], h["dots_cap"], h["qg"]) != S.plan_groups(S.G_NB[: r.cut], h["dots_cap"], h["qg"], strict=True):
            out.append(r.name)
    assert "cap70_c9" in out and "cap69_c9" not in out
    return out


WRONG = [("the split at nb / 2", "rows-u16_f16", _split_differs),
         ("chunk counts rounded down", "rows-u16_f16", lambda n: _dots_differ(n, round_up=False)),
         ("chunk counts rounded down", "chunks-u32_f16", lambda n: _dots_differ(n, round_up=False)),
         ("the owner search takes the first row with an equal prefix", "rows-u16_f16", lambda n: _dots_differ(n, owner="first")),
         ("the owner search takes the first row with an equal prefix", "chunks-u16_f16", lambda n: _dots_differ(n, owner="first")),
         ("the last chunk's count taken as 64", "chunks-u16_f16", lambda n: _dots_differ(n, last64=True)),
         ("the last chunk's count taken as 64", "rows-u32_f16", lambda n: _dots_differ(n, last64=True)),
         ("no carry across 64 components", "rows-u16_f16", lambda n: _dots_differ(n, carry=False)),
         ("no carry across 64 components", "pairs-u32_f16", lambda n: _dots_differ(n, carry=False)),
         ("descending order of additions", "rows-u32_f16", lambda n: _dots_differ(n, descending=True)),
         ("descending order of additions", "pairs-u16_f16", lambda n: _dots_differ(n, descending=True)),
         ("ties in select_lists by descending component", "select-u16_f16", _ties_differ),
         ("the group test with < for <=", "groups-u16_f16", _groups_differ)]


@pytest.mark.parametrize("reading,name,catch", WRONG, ids=["%s [%s]" % (r, n) for r, n, _ in WRONG])
def test_a_wrong_reading_is_caught(reading, name, catch):
    caught = catch(name)
    print("wrong reading %r: caught by %s %s" % (reading, name, caught[:6]))
    assert len(caught) >= 1, reading


def test_a_weakened_collection_fails_its_check():
    """Halving the target lists' postings prunes them: the row halves no longer hold, and check() says so."""
    case = S.make("rows-u16_f16")
    weak = S.Case.__new__(S.Case)
    weak.__dict__.update(case.__dict__)
    weak.cfg = dict(case.cfg, n_postings=150)
    with pytest.raises(AssertionError):
        weak.check(weak.build())
    assert SC.FORMS[case.form] == (2, 0)
