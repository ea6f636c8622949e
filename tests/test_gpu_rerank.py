"""sgpu_rerank_documents on the device: rows bit-identical to the host twin and to the oracle's rows (out_n, ids, score
bits, zero padding) on tests/score_cases.py; candidate counts around k and the chunk size C with the merge rounds
counted; launch cuts inside a query's candidates; both lookup forms; a second replica; the device-side checks; beside a
searching thread; the Python classes."""
import ctypes as C
import threading

import numpy as np
import pytest

import rerank_cases
import score_cases
import seismic_amd
from rerank_cases import assert_rows, expected_rows
from seismic_amd import _native

pytestmark = pytest.mark.gpu

KS = (1, 10, 1024)
EDEVICE = 2


def _stats(ix, replica=0):
    """sgpu_debug_score_stats: score kernel ms, launches, ..., selection ms, merge rounds."""
    out = np.zeros(8, np.float64)
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    _native.check(L.sgpu_debug_score_stats(ix.h, replica, out.ctypes.data_as(C.c_void_p)))
    return dict(ms=out[0], launches=int(out[1]), dense=int(out[2]), select_ms=out[6], rounds=int(out[7]))


def _rounds(n, chunk, k):
    """Merge rounds of one query of n candidates in one launch: its ceil(n / C) chunk survivors merged floor(C / k) at a time."""
    cnt, fan, r = -(-n // chunk), chunk // k, 0
    if cnt <= 1:
        return 0
    while True:
        r += 1
        if cnt <= fan:
            return r
        cnt = -(-cnt // fan)


_UPLOADED = {}


@pytest.fixture(scope="module")
def uploaded():
    """One upload per case, shared by the tests of this file."""
    def get(name):
        if name not in _UPLOADED:
            _UPLOADED[name] = score_cases.make(name).build().upload(0)
        return _UPLOADED[name]
    yield get
    for ix in _UPLOADED.values():
        ix.close()
    _UPLOADED.clear()


def _both(case, ix, q_off, qc, qv, cand_off, cand_ids, k, want, what, replica=0):
    """The device's rows and the host twin's against the oracle's."""
    assert_rows(ix.rerank_documents_host(q_off, qc, qv, cand_off, cand_ids, k), want, what + " (host)")
    assert_rows(ix.rerank_documents(q_off, qc, qv, cand_off, cand_ids, k, replica=replica), want, what + " (device)")


def _one_query(case, q):
    a, b = int(case.q_off[q]), int(case.q_off[q + 1])
    return np.array([0, b - a], np.uint64), case.qc[a:b], case.qv[a:b]


def _every_document_three_times(case):
    ids = np.random.default_rng(31).permutation(np.tile(np.arange(case.n_docs, dtype=np.uint64), 3))
    assert len(ids) == 6000
    return np.array([0, len(ids)], np.uint64), ids


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", sorted(score_cases.CASES))
def test_device_equals_host_twin_equals_oracle(name, k, uploaded):
    rerank_cases.assert_discriminates(KS)   # (the oracle alone, before the library is looked at; cached)
    case, ix = score_cases.make(name), uploaded(name)
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    _both(case, ix, case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k, want, "%s k=%d" % (name, k))
    st = _stats(ix)
    assert st["launches"] == 1 and st["rounds"] == 0 and st["select_ms"] > 0   # (2000 candidates at most: one chunk each)
    # no candidate at all, and no query: SGPU_OK; zeroed rows
    zero = np.zeros(score_cases.N_QUERIES + 1, np.uint64)
    sc, ids, n = ix.rerank_documents(case.q_off, case.qc, case.qv, zero, np.zeros(0, np.uint64), k)
    assert sc.shape == (score_cases.N_QUERIES, k) and not sc.view(np.uint32).any() and not ids.any() and not n.any()
    assert len(ix.rerank_documents(np.zeros(1, np.uint64), case.qc, case.qv, np.zeros(1, np.uint64), np.zeros(0, np.uint64), k)[2]) == 0


@pytest.mark.parametrize("small_k", [False, True])
@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("name", ["u16_f16", "u16_dvb_small"])
def test_candidate_counts_around_k_and_the_chunk(name, chunk, small_k, uploaded, monkeypatch):
    """C = `chunk` through the test hook. k = C / 2 merges two slots at a time (up to three rounds at these sizes); k = 5
    merges all of them in one round. Every list once with distinct ids and once with every id three times, in shuffled positions."""
    case, ix = score_cases.make(name), uploaded(name)
    k = 5 if small_k else chunk // 2
    monkeypatch.setenv("SGPU_RERANK_CHUNK", str(chunk))
    rng = np.random.default_rng(chunk + k)
    seen = set()
    for j, n in enumerate((k - 1, k, k + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1)):
        distinct = rng.choice(case.n_docs, n, replace=False).astype(np.uint64)
        for ids in (distinct, rng.permutation(np.tile(distinct, 3))):
            q = (2, 8, 9, 1)[j % 4]   # (300 components; two ordinary queries; one component: thousands of +0.0 ties)
            q_off, qc, qv = _one_query(case, q)
            off = np.array([0, len(ids)], np.uint64)
            want = expected_rows(case, off, ids, k, queries=[q])
            assert want[2][0] == min(k, n)
            _both(case, ix, q_off, qc, qv, off, ids, k, want, "%s C=%d k=%d n=%d x%d" % (name, chunk, k, n, len(ids) // n))
            st = _stats(ix)
            assert st["rounds"] == _rounds(len(ids), chunk, k), (n, len(ids), st)
            seen.add(st["rounds"])
    assert seen == ({0, 1} if small_k else {0, 1, 2, 3}), seen   # the test reached the merge, at every depth


def test_a_k_above_half_the_hooked_chunk_raises_it(uploaded, monkeypatch):
    case, ix = score_cases.make("u16_f16"), uploaded("u16_f16")
    monkeypatch.setenv("SGPU_RERANK_CHUNK", "64")
    off, ids = _every_document_three_times(case)
    q_off, qc, qv = _one_query(case, 2)
    for k, c in ((33, 128), (100, 256)):   # C = 2 * next_pow2(k)
        _both(case, ix, q_off, qc, qv, off, ids, k, expected_rows(case, off, ids, k, queries=[2]), "k=%d" % k)
        assert _stats(ix)["rounds"] == _rounds(6000, c, k)


@pytest.mark.parametrize("k", [10, 1024])
@pytest.mark.parametrize("name", ["u16_f16", "u16_dvb_small", "u32_u8"])
def test_every_document_three_times_with_the_default_chunk(name, k, uploaded):
    case, ix = score_cases.make(name), uploaded(name)
    off, ids = _every_document_three_times(case)
    for q in (0, 2, 9):   # (the empty query: 2000 ties at +0.0)
        q_off, qc, qv = _one_query(case, q)
        _both(case, ix, q_off, qc, qv, off, ids, k, expected_rows(case, off, ids, k, queries=[q]), "%s q%d k=%d" % (name, q, k))
        assert _stats(ix)["rounds"] == _rounds(6000, 2048, k) == (1 if k == 10 else 2)


@pytest.mark.parametrize("cut", [7, 128, 1000])
@pytest.mark.parametrize("name", ["u16_f16", "u16_dvb_small"])
def test_launch_cuts_change_no_row(name, cut, uploaded, monkeypatch):
    """SGPU_SCORE_CHUNK cuts the call into launches of `cut` candidates: duplicates of one id lie on both sides of a cut and
    a query's candidates span many launches; its survivors wait in the carry slots."""
    case, ix = score_cases.make(name), uploaded(name)
    off3, ids3 = _every_document_three_times(case)
    q_off3, qc3, qv3 = _one_query(case, 9)
    for k in (3, 1024):
        uncut = ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k)
        assert _stats(ix)["launches"] == 1
        uncut3 = ix.rerank_documents(q_off3, qc3, qv3, off3, ids3, k)
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(cut))
        got = ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k)
        st = _stats(ix)
        got3 = ix.rerank_documents(q_off3, qc3, qv3, off3, ids3, k)
        st3 = _stats(ix)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        assert st["launches"] == -(-len(case.cand_ids) // cut) and st3["launches"] == -(-6000 // cut) and st3["rounds"] >= st3["launches"] - 1
        want = expected_rows(case, case.cand_off, case.cand_ids, k)
        want3 = expected_rows(case, off3, ids3, k, queries=[9])
        assert_rows(uncut, want, "uncut")
        assert_rows(got, want, "%s cut %d k=%d" % (name, cut, k))
        assert_rows(uncut3, want3, "uncut, 6000 entries")
        assert_rows(got3, want3, "%s cut %d k=%d, 6000 entries" % (name, cut, k))


def test_launch_cuts_and_a_small_chunk_together(uploaded, monkeypatch):
    case, ix = score_cases.make("u16_dvb_small"), uploaded("u16_dvb_small")
    monkeypatch.setenv("SGPU_RERANK_CHUNK", "64")
    monkeypatch.setenv("SGPU_SCORE_CHUNK", "1000")   # (15 chunks and a rest per launch; every query over 2 launches or more)
    k = 20
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want)
    assert _stats(ix)["launches"] == -(-len(case.cand_ids) // 1000)


def test_the_lookup_form_changes_no_row(uploaded, monkeypatch):
    case, ix = score_cases.make("u16_f16_small"), uploaded("u16_f16_small")
    k = 10
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want, "hash")
    assert _stats(ix)["dense"] == 0
    monkeypatch.delenv("SGPU_SCORE_LOOKUP")
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want, "dense")
    assert _stats(ix)["dense"] == 1


def test_a_second_replica_on_the_same_device():
    case = score_cases.make("u16_u8")
    ix = case.build()
    ix.upload_many([0, 0])
    k = 10
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k, replica=1), want, "replica 1")
    assert _stats(ix, 1)["launches"] == 1
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k, replica=0), want, "replica 0")
    ix.close()


def test_device_side_checks_leave_the_index_usable():
    case = score_cases.make("u32_f16")
    ix = case.build()
    k = 3
    with pytest.raises(_native.SeismicHipError) as e:   # not uploaded
        ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k)
    assert e.value.status == EDEVICE and "not uploaded" in str(e.value)
    ix.upload(0)
    with pytest.raises(_native.SeismicHipError) as e:   # replica out of range
        ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k, replica=1)
    assert e.value.status == EDEVICE
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want)
    # ... and rerank calls take turns with score calls on the replica's scratch
    sc = ix.score_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
    assert np.array_equal(sc.view(np.uint32), case.expected(case.cand_off, case.cand_ids))
    assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want)
    ix.close()


def test_reranking_beside_a_searching_thread(uploaded):
    case, ix = score_cases.make("u16_f16"), uploaded("u16_f16")
    k = 10
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    want_search = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
    errors, done = [], threading.Event()

    def rerank():
        try:
            for _ in range(20):
                assert_rows(ix.rerank_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want)
        except Exception as e:   # noqa: BLE001 (reported by the test's thread)
            errors.append(repr(e))
        finally:
            done.set()

    def search():
        rounds = 0
        while not done.is_set() or rounds < 3:
            sc, ids, n = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")
            rounds += 1
            if rounds >= 1000:
                break

    threads = [threading.Thread(target=rerank), threading.Thread(target=search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]


@pytest.mark.parametrize("k", [3, 100])
def test_python_batch_rerank_on_the_device_equals_the_host(k):
    case = score_cases.make("u16_dvb")
    ix = seismic_amd.SeismicIndexRaw(case.build(), device=0)
    qcs = [c for c, _ in case.queries]
    qvs = [v for _, v in case.queries]
    dev = ix.batch_rerank(qcs, qvs, case.lists, k)
    assert dev == ix.batch_rerank(qcs, qvs, case.lists, k, device=False)
    wb, wi, wn = expected_rows(case, case.cand_off, case.cand_ids, k)
    assert [[d for _, d in row] for row in dev] == [wi[q, :wn[q]].tolist() for q in range(len(wn))]
    assert ix.rerank(qcs[2], qvs[2], case.lists[2], k) == dev[2] == ix.rerank(qcs[2], qvs[2], case.lists[2], k, device=0)
    with pytest.raises(ValueError):
        ix.rerank(qcs[2], qvs[2], case.lists[2], k, device=1)
