"""The reference side of tests/test_gpu_exact_edges.py, without a device: on every case of tests/exact_cases.py the case
has the property it exists for (check()), host exact search equals the oracle's sequential brute force bit for bit and
satisfies the float64 model's checkers with the model's own bounds, and a numpy restatement of exact search equals the
host - while each deliberately wrong restatement (segments cut at one step, the first 256 query components only,
descending component order, a scan without the carry between tiles, ties by descending id) disagrees with it on that
case's queries: the inputs can see that class of bug."""
import functools

import numpy as np
import pytest

import exact_cases as EC
import model64 as M64
import orc

ORACLE_KS = (1, 10, 100)


@functools.lru_cache(maxsize=None)
def _built(name, vt):
    """(case, host index, descriptor arrays, model, restatement) of a variant; nothing is uploaded."""
    case = EC.make(name)
    ix = case.build(vt)
    d = ix.desc
    arrays = orc.desc_arrays(d)
    return case, ix, arrays, M64.Model(arrays, d.val_scale, d.value_type), EC.Restated(arrays, d.val_scale, d.value_type, case.dim)


def _row(rows, i):
    s, ids, n = rows
    return s[i, :int(n[i])], ids[i, :int(n[i])]


def _same_row(a, b):
    return len(a[0]) == len(b[0]) and np.array_equal(a[1], b[1]) and \
        np.array_equal(np.asarray(a[0], np.float32).view(np.uint32), np.asarray(b[0], np.float32).view(np.uint32))


def test_the_forward_only_configuration_is_test_gpu_exacts():
    import inspect

    import test_gpu_exact
    src = inspect.getsource(test_gpu_exact._forward_only)
    for key, value in EC.FORWARD_ONLY.items():
        assert "%s=%r" % (key, value) in src, key


@pytest.mark.parametrize("variant", EC.VARIANTS, ids=EC.VARIANT_IDS)
def test_case_has_its_property_and_host_equals_oracle_model_and_restatement(variant):
    case, ix, arrays, model, rest = _built(*variant)
    found = case.check(arrays)
    print("exact case %s-vt%d: %s -> %s" % (variant + (case.paths, found)))
    assert ix.desc.n_docs == case.n_docs and ix.desc.value_type == variant[1]
    nq = len(case.queries)
    # host == oracle (ORDER_SEQ: the plain left-to-right sum), bit for bit
    for k in ORACLE_KS:
        host = ix.exact_search(case.q_off, case.qc, case.qv, k)
        assert (host[2] == min(k, case.n_docs)).all()
        for i, (c, v) in enumerate(case.queries):
            assert _same_row(_row(host, i), orc.exact_search(ix.desc, c, v, k, orc.ORDER_SEQ)), (k, i)
    # host == the numpy restatement, at the largest k
    host = ix.exact_search(case.q_off, case.qc, case.qv, EC.MAX_K)
    for i, (c, v) in enumerate(case.queries):
        assert _same_row(_row(host, i), rest.topk(rest.scores(c, v), EC.MAX_K)), i
    # the model's checkers on a sample of the queries, with its own bounds
    tally, worst = M64.Tally(), 0.0
    for k in (10, EC.MAX_K):
        rows = host if k == EC.MAX_K else ix.exact_search(case.q_off, case.qc, case.qv, k)
        for i in sorted(set(range(0, nq, 3)) | {nq - 1}):
            q = model.query(*case.queries[i], index=i)
            s, ids = _row(rows, i)
            model.check_rows(rows[0][i], rows[1][i], rows[2][i], k, i)
            worst = max(worst, model.check_scores(q, ids, s))
            tally.add(model.check_topk(q, ids, s, None, k))
    print("model64: %-34s unambiguous=%s score_ratio=%.4g" % ("host exact %s-vt%d" % variant, tally, worst))


def _differs(variant, k=EC.MAX_K, ties_descending=False, **wrong):
    """The queries of the variant on which the wrong restatement's top-k is not the host's."""
    case, ix, _, _, rest = _built(*variant)
    host = ix.exact_search(case.q_off, case.qc, case.qv, k)
    out = []
    for i, (c, v) in enumerate(case.queries):
        assert _same_row(_row(host, i), rest.topk(rest.scores(c, v), k)), i      # (the right reading agrees)
        if not _same_row(_row(host, i), rest.topk(rest.scores(c, v, **wrong), k, ties_descending=ties_descending)):
            out.append(i)
    return out


@pytest.mark.parametrize("vt", [0, 1])
def test_segments_cut_at_one_step_are_seen(vt):
    seen = _differs(("segments", vt), segment_cap=EC.STEP)
    # the components of 16 384 ... 32 768 entries and the 9000 of range 1 alone, and all the heavy ones together (queries 2
    # and 8 - 8193 entries - lose one document's entry: the top-k need not show it, the score vectors below do)
    assert {3, 4, 5, 6, 7, 9, 10} <= set(seen), seen
    assert not {0, 1, 12, 15} & set(seen), seen      # 8191 and 8192 entries are one step: nothing is cut
    case, _, _, _, rest = _built("segments", vt)
    for i in (2, 8):
        c, v = case.queries[i]
        assert (rest.scores(c, v).view(np.uint32) != rest.scores(c, v, segment_cap=EC.STEP).view(np.uint32)).sum() == 1


@pytest.mark.parametrize("name", ["long_u16", "long_u32"])
def test_only_the_first_256_query_components_are_seen(name):
    seen = _differs((name, 0), max_comps=EC.GROUP)
    assert {4, 5, 6, 7, EC.LONG_Q_GROUP, EC.LONG_Q_255_256} <= set(seen), seen        # 511 components and more, absent groups
    assert not {0, 1, 2, EC.LONG_Q_LAST} & set(seen), seen                              # 0, 255, 256, 41


@pytest.mark.parametrize("variant", [("segments", 0), ("long_u16", 0), ("long_u32", 0), ("documents", 0)])
def test_descending_component_order_is_seen(variant):
    seen = _differs(variant, descending=True)
    assert len(seen) >= 3, seen


@pytest.mark.parametrize("dim", EC.SCAN_DIMS)
def test_a_scan_without_the_carry_between_tiles_is_seen(dim):
    case, _, arrays, _, _ = _built("scan_%d" % dim, 0)
    cnt = EC.segment_counts(arrays, dim)
    seen = []
    for r in range(cnt.shape[0]):
        row = np.append(cnt[r], 0)
        true = EC.scan_offsets(row)
        assert np.array_equal(true, np.cumsum(row) - row) and true[-1] == cnt[r].sum()
        wrong = EC.scan_offsets(row, carry=False)
        # a query component sees it where its segment's begin or end differs
        seen += [c for c in sorted(set(case.qc.tolist())) if wrong[c] != true[c] or wrong[c + 1] != true[c + 1]]
    if dim + 1 <= EC.TILE:
        assert not seen          # one tile: there is no carry to drop (4095 and 4096 counts fill it up to and at its edge)
    else:
        assert dim - 1 in seen and len(seen) >= 2, seen


def test_ties_by_descending_id_are_seen():
    assert _differs(("ties", 0), k=10, ties_descending=True) == [0, 1, 2]
    assert _differs(("ties", 0), ties_descending=True) == [0, 1, 2]


@pytest.mark.parametrize("kf", EC.TIES_KS)
def test_ties_under_filters_on_the_host(kf):
    """Host filtered exact search on the ties case is what reasoning alone says: the allowed holders by ascending id, then
    the allowed empty documents (or the other way round under the negative query)."""
    case, ix, arrays, _, rest = _built("ties", 0)
    filters = EC.tie_filters(kf)
    print("tie filters k=%d, allowed per range: %s" % (kf, EC.check_tie_filters(kf, filters)))
    for name, allowed in filters.items():
        f = ix.make_filter(allowed)
        for k in (1, 64, 1024):
            host = ix.exact_search(case.q_off, case.qc, case.qv, k, filter=f)
            assert (host[2] == min(k, len(allowed))).all(), (name, k)
            for i in range(3):
                assert _same_row(_row(host, i), EC.ties_expected(i, k, allowed)), (name, k, i)
                assert not host[1][i, int(host[2][i]):].any()
    # unfiltered too
    for k in (1, 64, 1024):
        host = ix.exact_search(case.q_off, case.qc, case.qv, k)
        for i in range(3):
            assert _same_row(_row(host, i), EC.ties_expected(i, k)), (k, i)
