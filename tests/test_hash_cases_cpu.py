"""The cases of tests/hash_cases.py reach their edges, the library's seed search (sgpu_debug_plan_seeds: make_plan through
the debug_plan path) equals the restatement seed for seed and hash_ok for hash_ok on every batch of both vocabularies, hash_ok
is 0 for every index form that has no hashed kernels, and the launch configuration's hook takes the hashed lookup exactly
when hash_ok is set. No GPU. The GPU half: test_gpu_hash_lookup.py, which imports the shared pieces from here."""
import functools

import numpy as np
import pytest

import coop_cases as CC
import hash_cases as H
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

SGPU_ELIMIT = 5


@functools.lru_cache(maxsize=None)
def built(vocab):
    """(case, host index) - once per process."""
    case = H.make(vocab)
    return case, case.build()


@functools.lru_cache(maxsize=None)
def graph(vocab):
    """The kNN graph of a vocabulary's index (the oracle's Knn::new)."""
    return orc.knn_build(built(vocab)[1].desc, H.KNN)


@functools.lru_cache(maxsize=None)
def oracle_counts(vocab, run_name):
    """(scores, ids, n, counts) of a run's DISTINCT queries, each on its own."""
    case, ix = built(vocab)
    run = case.runs[run_name]
    Q = orc.csr([case.queries[n] for n in run.queries])
    return orc.batch_search_counts(ix.desc, *Q, run.k, run.cut, run.hf, run.first_sorted)


def launches():
    """Every (variant name, block, environment, hook mode) a batch is launched under through a resident batch."""
    out = [(v, b, dict(env, SGPU_BLOCK=str(b)), 0) for v, env in H.VARIANTS.items() for b in H.BLOCKS]
    return out + [("counted", 512, dict(SGPU_BLOCK="512"), 2)]


def launch_env(run, env):
    """A variant's environment with the run's own knobs."""
    return dict(env, **run.env)


def expectation(case, ix, run, env, mode=0, **chip):
    """(hash_ok by the restatement, the hook's words for the launch told so - or None where the hook says the launch cannot
    be configured: SGPU_ELIMIT, no lookup layout fits the LDS)."""
    ok, _ = case.restated(run, no_hash=env.get("SGPU_NO_HASH") == "1")
    try:
        return ok, H.hook(case, ix, run, env, ok, mode=mode, **chip)
    except _native.SeismicHipError as e:
        assert e.status == SGPU_ELIMIT, e
        return ok, None


@pytest.mark.parametrize("vocab", H.VOCABS + ("wide",))
def test_the_cases_reach_their_edges(vocab):
    found = H.make(vocab).check()
    print(vocab, found)
    assert found["padded_mate_documents"] >= H.N_MATES // 3 and found["wrong_score_margin_in_bounds"] > 8


@pytest.mark.parametrize("vocab", H.VOCABS)
def test_the_mate_documents_are_in_the_oracles_row(vocab):
    case, ix = built(vocab)
    sc, ids, n, _ = oracle_counts(vocab, "mates")
    row = ids[0, : n[0]].astype(np.int64)
    assert n[0] == case.runs["mates"].k and np.isin(np.arange(H.N_DOCS, H.N_DOCS + H.N_MATES), row).all()


@pytest.mark.parametrize("vocab", H.VOCABS)
def test_the_librarys_seeds_are_the_restatements(vocab):
    case, ix = built(vocab)
    for run in case.runs.values():
        Q = case.batch(run)
        ok, seeds = _native.debug_plan_seeds(ix, *Q, run.cut)
        want_ok, want = case.restated(run)
        assert ok == want_ok, (vocab, run.name, ok, want_ok)
        bad = np.flatnonzero(seeds != want)
        assert len(bad) == 0, (vocab, run.name, int(bad[0]), int(seeds[bad[0]]), int(want[bad[0]]))
        # every query on its own: its seed, or hash_ok == 0 and the entry 64 & 63
        for name in run.queries:
            q = orc.csr([case.queries[name]])
            ok1, s1 = _native.debug_plan_seeds(ix, *q, run.cut)
            s = H.query_seed(case.queries[name][0])
            assert (ok1, int(s1[0])) == ((1, s) if s < H.HASH_SEEDS else (0, 0)), (vocab, name, ok1, s1, s)


def test_hash_ok_is_zero_without_hashed_kernels(monkeypatch):
    case, ix = built("small")
    runs = [case.runs[n] for n in ("sizes", "cycle", "alone", "mates")]
    for run in runs:
        assert _native.debug_plan_seeds(ix, *case.batch(run), run.cut)[0] == 1, run.name
    # dim == 2^24: the same documents and queries as `large`, one id more in the vocabulary
    wide, wix = built("wide")
    assert wix.desc.dim == 1 << 24
    for run in (wide.runs[n] for n in ("sizes", "cycle", "alone", "mates")):
        ok, seeds = _native.debug_plan_seeds(wix, *wide.batch(run), run.cut)
        assert ok == 0 and not seeds.any(), run.name
        assert wide.restated(run)[0] == 0
    # fixed-u8 values over u32 components
    u8 = ix.convert(1)
    for run in runs:
        ok, seeds = _native.debug_plan_seeds(u8, *case.batch(run), run.cut)
        assert ok == 0 and not seeds.any(), run.name
        assert H.seeds(*case.batch(run)[:2], case.dim, 4, 1)[0] == 0
    # u16 components
    rng = np.random.default_rng(5)
    docs = [(np.sort(rng.choice(3000, 12, replace=False)), np.full(12, 0.5, np.float32)) for _ in range(60)]
    u16 = _native.NativeIndex.build(2, 3000, *orc.csr(docs), BuildConfig.defaults(n_postings=100))
    q = orc.csr([docs[0], docs[1], (np.array([7]), np.array([1.0], np.float32))])
    for form in (u16, u16.convert(1), u16.convert(2)):
        ok, seeds = _native.debug_plan_seeds(form, *q, 3)
        assert ok == 0 and not seeds.any()
    assert H.seeds(*q[:2], 3000, 2, 0)[0] == 0
    # SGPU_NO_HASH
    monkeypatch.setenv("SGPU_NO_HASH", "1")
    for run in runs:
        ok, seeds = _native.debug_plan_seeds(ix, *case.batch(run), run.cut)
        assert ok == 0 and not seeds.any(), run.name
        assert case.restated(run, no_hash=True)[0] == 0


@pytest.mark.parametrize("vocab", H.VOCABS)
def test_the_hook_takes_the_hashed_lookup_exactly_when_hash_ok_is_set(vocab):
    case, ix = built(vocab)
    seen = {}
    for run in case.runs.values():
        for variant, block, env, mode in launches():
            env = launch_env(run, env)
            ok, h = expectation(case, ix, run, env, mode)
            key = (vocab, run.name, variant, block)
            if ok and (vocab, run.name) not in H.LDS_DECLINES:
                assert h is not None and h["lookup"] == H.LK_HASH and h["lds_bytes"] <= 160 * 1024, (key, h)
            elif ok:
                assert h is not None and h["lookup"] == 2, (key, h)         # (named: the LDS fitting declines it; split fits)
            elif vocab == "large":
                assert h is None, (key, h)                                  # no fallback layout fits 2^24 - 1 ids
            else:
                assert h is not None and h["lookup"] in (0, 2), (key, h)    # packed or split
            # told the opposite, the hook answers the opposite: hash_ok is what decides
            with CC.knobs(env):
                if ok:
                    try:
                        other = H.hook(case, ix, run, env, 0, mode=mode)["lookup"]
                    except _native.SeismicHipError:
                        other = None
                    assert other != H.LK_HASH, key
            seen[key] = None if h is None else h["lookup"]
    print(vocab, sorted(set((k[1], v) for k, v in seen.items()), key=str))
    with CC.knobs(dict(SGPU_NO_HASH="1")):
        for run in case.runs.values():
            try:
                assert H.hook(case, ix, run, dict(SGPU_NO_HASH="1"), 1)["lookup"] != H.LK_HASH, run.name
            except _native.SeismicHipError as e:
                assert vocab == "large" and e.status == SGPU_ELIMIT
