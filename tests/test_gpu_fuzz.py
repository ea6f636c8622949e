"""Seeded differential fuzzing: random datasets / build parameters / search parameters, GPU vs oracle,
bit-exact. Includes tie-heavy data (values from a tiny set), negative weights, k around the 64-lane
register boundaries, heap_factor 0 and > 1, sorted / unsorted, kNN refinement."""
import numpy as np
import pytest

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import desc_equal

pytestmark = pytest.mark.gpu


def _dataset(rng, n_docs, dim, nnz_lo, nnz_hi, values):
    vecs = []
    for d in range(n_docs):
        if rng.random() < 0.02:
            vecs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        n = int(rng.integers(nnz_lo, min(nnz_hi, dim) + 1))
        c = np.sort(rng.choice(dim, n, replace=False)).astype(np.uint32)
        vecs.append((c, values(rng, n)))
    return orc.csr(vecs)


def _queries(rng, nq, dim, nnz_hi, values):
    vecs = []
    for _ in range(nq):
        n = int(rng.integers(0, min(nnz_hi, dim) + 1))
        c = np.sort(rng.choice(dim, n, replace=False)).astype(np.uint32)
        vecs.append((c, values(rng, n)))
    return orc.csr(vecs)


VALUE_LAWS = {
    "exp": lambda rng, n: (rng.exponential(0.5, n) + 0.01).astype(np.float32),
    "ties": lambda rng, n: rng.choice([0.5, 1.0, 2.0], n).astype(np.float32),
    "signed": lambda rng, n: rng.normal(0, 1, n).astype(np.float32),
}


def _collection(seed, law):
    """The seed's documents and build configuration (and the generator, for what the caller draws next)."""
    rng = np.random.default_rng(1000 + seed)
    values = VALUE_LAWS[law]
    cw = 4 if seed % 5 == 4 else 2
    dim = int(rng.choice([24, 100, 700, 3000])) if cw == 2 else int(rng.choice([70000, 150000]))
    n_docs = int(rng.integers(60, 2500))
    docs = _dataset(rng, n_docs, dim, 1, int(rng.choice([8, 40, 200, 400])), values)
    cfg = dict(n_postings=int(rng.choice([1, 3, 20, 200])), centroid_fraction=float(rng.choice([0.02, 0.1, 0.3, 0.6])),
               summary_energy=float(rng.choice([0.2, 0.5, 0.9, 1.0])), max_fraction=float(rng.choice([1.0, 1.5, 6.0])),
               min_cluster_size=int(rng.integers(0, 6)), doc_cut=int(rng.choice([1, 5, 15])))
    return rng, values, cw, dim, docs, cfg


@pytest.mark.parametrize("law", ["exp", "ties", "signed"])
@pytest.mark.parametrize("seed", range(14, 26))
def test_device_build_laws(seed, law):
    """The device-assisted build of the differential seeds' collections under every value law (test_differential builds
    on the device only where the law is "exp"): byte-identical to the host builder's index."""
    _, _, cw, dim, docs, cfg = _collection(seed, law)
    host = _native.NativeIndex.build(cw, dim, *docs, BuildConfig.defaults(**cfg))
    dev = _native.NativeIndex.build(cw, dim, *docs, BuildConfig.defaults(use_device=1, **cfg))
    desc_equal(host.desc, dev.desc)


# (launches of 30 queries are cooperative ones by default - the round loop; "plain" switches that variant off, so the
# same seeds run the plain variants: stage 2 as a stream, 1024-thread workgroups on even seeds, 512 on odd ones)
@pytest.mark.parametrize("variant", ["default", "plain"])
@pytest.mark.parametrize("seed", range(26))
def test_differential(seed, variant, monkeypatch):
    differential(seed, variant, monkeypatch)


def differential(seed, variant, monkeypatch):
    """One seed's differential run; returns (index, queries) for callers that look at the launches it made."""
    if variant == "plain":
        monkeypatch.setenv("SGPU_COOP", "0")
    # small batches default to 1024-thread workgroups; odd seeds force the 512-thread configuration
    if seed % 2:
        monkeypatch.setenv("SGPU_BLOCK", "512")
    # seeds >= 14 also vary the round-2 machinery: fixed-u8 document values, lists walked one per
    # group, the document-major forward store, the device-assisted build, two replicas, large k
    if seed >= 14 and seed % 4 == 1:
        monkeypatch.setenv("SGPU_DOTS_CAP", "1")
    if seed >= 14 and seed % 4 == 2:
        monkeypatch.setenv("SGPU_FWD_LAYOUT", "doc")
    law = ["exp", "ties", "signed"][seed % 3]
    rng, values, cw, dim, (off, comps, vals), cfg = _collection(seed, law)
    if seed >= 14 and seed % 3 == 0:
        cfg["use_device"] = 1
    ix = _native.NativeIndex.build(cw, dim, off, comps, vals, BuildConfig.defaults(**cfg))
    if cfg.get("use_device") == 1:   # the index searched below is the host builder's, bit for bit
        host = _native.NativeIndex.build(cw, dim, off, comps, vals, BuildConfig.defaults(**dict(cfg, use_device=0)))
        desc_equal(host.desc, ix.desc)
        del host
    if seed >= 14 and seed % 2 == 0:
        # fixed-u8 document values (negative weights quantise to 0), u16 and u32 components; every other such seed with
        # u16 components also compresses the component stream (DotVByte forward index: lossless, same results)
        ix = ix.convert(2 if (cw == 2 and seed % 4 == 0) else 1)
    if seed >= 14 and seed % 5 == 0:
        ix.upload_many([0, 0])                  # two replicas: batches are sharded over them
    else:
        ix.upload(0)
    graph = None
    if seed % 2 == 0:
        nknn = int(rng.integers(1, 6))
        graph = orc.knn_build(ix.desc, nknn)
        ix.set_knn(graph, nknn)
        orc.knn_attach(graph, nknn)
    try:
        q = _queries(rng, 30, dim, int(rng.choice([5, 40, 120])), values)
        for _ in range(4):
            k = int(rng.choice([1, 3, 10, 63, 64, 65, 128, 129, 300] + ([256, 257, 513, 1000] if seed >= 14 else [])))
            qcut = int(rng.integers(1, 13))
            hf = float(rng.choice([0.0, 0.5, 0.8, 1.0, 1.3]))
            srt = bool(rng.integers(0, 2))
            n_knn = int(rng.integers(0, 8)) if graph is not None else 0
            gs, gi, gn = ix.batch_search(*q, k, qcut, hf, srt, n_knn=n_knn)
            cs, ci, cn, _, _, _ = orc.batch_search(ix.desc, *q, k, qcut, hf, srt, n_knn=n_knn)
            ctx = (seed, law, cfg, k, qcut, hf, srt, n_knn)
            assert np.array_equal(gn, cn), ctx
            for i in range(len(gn)):
                n = int(gn[i])
                assert np.array_equal(gi[i, :n], ci[i, :n]), (ctx, i, gi[i, :n], ci[i, :n], gs[i, :n], cs[i, :n])
                assert np.array_equal(gs[i, :n].view(np.uint32), cs[i, :n].view(np.uint32)), (ctx, i)
    finally:
        orc.knn_attach(None, 0)
    return ix, q


def test_long_summary_rows_and_long_queries():
    """Stage 1 edge cases: summary rows of thousands of entries (more than 64 chunks of 64 per
    wavefront, so the chunk-descriptor block is refilled), one-block lists, and queries of more than
    64 components (more than one block of rows). Dots and searches bit-exact against the oracle."""
    rng = np.random.default_rng(77)
    dim, n_docs = 3000, 12000
    vecs = []
    for d in range(n_docs):   # three ubiquitous light components + a few heavy rare ones: ~9000 one-document blocks
        extra = rng.choice(np.arange(3, dim), int(rng.integers(2, 7)), replace=False)
        c = np.sort(np.concatenate([[0, 1, 2], extra])).astype(np.uint32)
        v = np.where(c < 3, rng.uniform(0.01, 0.05, len(c)), rng.uniform(1.0, 3.0, len(c))).astype(np.float32)
        vecs.append((c, v))
    off, comps, vals = orc.csr(vecs)
    cfg = BuildConfig.defaults(n_postings=n_docs, centroid_fraction=0.75, summary_energy=1.0, max_fraction=1.0,
                               min_cluster_size=0, doc_cut=10)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, cfg).upload(0)
    a = orc.desc_arrays(ix.desc)
    nb0 = int(a["list_block_start"][1] - a["list_block_start"][0])
    rows0 = a["row_ptr"][int(a["list_row_start"][0]): int(a["list_row_start"][1]) + 1]
    assert nb0 > 5000 and int(np.diff(rows0).max()) > 64 * 64 * 2, (nb0, np.diff(rows0).max())
    qs = []
    for n in (3, 10, 70, 150):
        c = np.sort(rng.choice(dim, n, replace=False)).astype(np.uint32)
        if 0 not in c:
            c[0] = 0
            c = np.unique(c)
        v = (rng.exponential(0.5, len(c)) + 0.01).astype(np.float32)
        v[0] = 9.0   # list 0 (the long rows) is walked first
        qs.append((c, v))
    for c, v in qs:
        for lst in (0, 1, 2, 5):
            g = ix.summary_distances(lst, c, v)
            o = orc.summary_distances(ix.desc, lst, c, v)
            assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), (lst, len(c))
    q = orc.csr(qs)
    for k, qcut, hf in ((10, 1, 1.0), (100, 1, 0.7), (5, 1, 0.0)):
        gs, gi, gn = ix.batch_search(*q, k, qcut, hf, False)
        cs, ci, cn, _, _, _ = orc.batch_search(ix.desc, *q, k, qcut, hf, False)
        assert np.array_equal(gn, cn)
        for i in range(len(gn)):
            n = int(gn[i])
            assert np.array_equal(gi[i, :n], ci[i, :n]), (k, qcut, hf, i)
            assert np.array_equal(gs[i, :n].view(np.uint32), cs[i, :n].view(np.uint32)), (k, qcut, hf, i)
