#!/usr/bin/env python3
"""sgpu_rerank_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index, against what a caller had before it: sgpu_score_documents and a
selection on the host. The workloads are tools/score_probe.py's:
  uniform   --queries queries x 100 candidates drawn uniformly, k = 10
  search    --queries queries x the ids each query's own search returns (k = 10, query_cut 4, heap_factor 1.0) plus
            random ids up to 100, k = 10 and k = 100
  one_query 1 query x 1 000 000 candidates drawn uniformly, k = 10 and k = 1000
Per workload and k, after 3 warm-up rounds, 20 timed rounds; a round runs the three paths one after the other (A B C A B C
...), so that they see the same box in the same state. One JSON line each with
  score_ms, select_ms   device time of a rerank call's score kernels and of its selection kernels (HIP events inside the
                        launcher: sgpu_debug_score_stats), medians; merge_rounds
  call_ms               the rerank call from host buffers to host rows (wall clock), median
  loop_ms               sgpu_score_documents + the per-query numpy loop (np.unique, stable np.argsort) that batch_rerank ran
                        before the native call - without building its Python tuples -, median; loop_score_ms: its score call
  vector_ms             sgpu_score_documents + one np.lexsort over (query, -score, id), a mask that drops repeats and a
                        rank cut: the selection without a Python loop, median
  bytes_to_host         nq x k x 12 + nq x 4 for the rerank call, 4 per candidate for the score call
  rows_equal            the three paths returned the same ids and score bits
The score path (score_documents_kernel, its launcher, sgpu_score_documents) is the same code before and after the rerank
call was added, so loop_ms and vector_ms are what the commit before it measures.

  python tools/rerank_probe.py > profiles/rerank_documents.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_score_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

WARMUP, TIMED = 3, 20


def stats(ix):
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(8, np.float64)
    _native.check(L.sgpu_debug_score_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return out


def select_loop(scores, cand_off, cand, k):
    """The per-query loop of batch_rerank before the native call."""
    nq = len(cand_off) - 1
    out_s, out_i, out_n = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)
    b = cand_off.astype(np.int64)
    for q in range(nq):
        ids, first = np.unique(cand[b[q]:b[q + 1]].astype(np.int64), return_index=True)
        s = scores[b[q]:b[q + 1]][first]
        order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        out_s[q, :len(order)], out_i[q, :len(order)], out_n[q] = s[order], ids[order], len(order)
    return out_s, out_i, out_n


def select_vector(scores, cand_off, cand, k):
    """The same rows without a Python loop: one lexsort, repeats dropped by a mask (equal ids of a query carry equal
    scores, so they are neighbours), ranks cut at k."""
    nq = len(cand_off) - 1
    out_s, out_i, out_n = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)
    qidx = np.repeat(np.arange(nq), np.diff(cand_off.astype(np.int64)))
    order = np.lexsort((cand, -scores, qidx))
    qs, ids = qidx[order], cand[order]
    keep = np.ones(len(order), bool)
    keep[1:] = (qs[1:] != qs[:-1]) | (ids[1:] != ids[:-1])
    order, qs = order[keep], qs[keep]
    rank = np.arange(len(order)) - np.searchsorted(qs, np.arange(nq))[qs]
    sel = rank < k
    out_s[qs[sel], rank[sel]] = scores[order[sel]]
    out_i[qs[sel], rank[sel]] = cand[order[sel]]
    out_n[:] = np.minimum(np.bincount(qs, minlength=nq), k)
    return out_s, out_i, out_n


def measure(ix, name, q, cand_off, cand, k):
    nq = len(q[0]) - 1
    t_new, t_loop, t_loop_score, t_vec, score_ms, select_ms = [], [], [], [], [], []
    st = rows = None
    for i in range(WARMUP + TIMED):
        t = time.perf_counter()
        a = ix.rerank_documents(q[0], q[1], q[2], cand_off, cand, k)
        w_new = (time.perf_counter() - t) * 1e3
        st = stats(ix)
        t = time.perf_counter()
        sc = ix.score_documents(q[0], q[1], q[2], cand_off, cand)
        w_score = (time.perf_counter() - t) * 1e3
        b = select_loop(sc, cand_off, cand, k)
        w_loop = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        sc = ix.score_documents(q[0], q[1], q[2], cand_off, cand)
        c = select_vector(sc, cand_off, cand, k)
        w_vec = (time.perf_counter() - t) * 1e3
        if i >= WARMUP:
            t_new.append(w_new), t_loop.append(w_loop), t_loop_score.append(w_score), t_vec.append(w_vec)
            score_ms.append(st[0]), select_ms.append(st[6])
        rows = a, b, c
    a, b, c = rows
    equal = all(np.array_equal(a[2], o[2]) and np.array_equal(a[1], o[1]) and
                np.array_equal(a[0].view(np.uint32), o[0].view(np.uint32)) for o in (b, c))
    med = lambda v: round(float(np.median(v)), 4)   # noqa: E731
    return {"workload": name, "queries": nq, "candidates": int(len(cand)), "k": k, "launches": int(st[1]),
            "merge_rounds": int(st[7]), "score_ms": med(score_ms), "select_ms": med(select_ms),
            "select_ms_min": round(float(np.min(select_ms)), 4), "select_ms_max": round(float(np.max(select_ms)), 4),
            "call_ms": med(t_new), "loop_ms": med(t_loop), "loop_score_ms": med(t_loop_score), "vector_ms": med(t_vec),
            "bytes_to_host": nq * k * 12 + nq * 4, "bytes_to_host_score_call": 4 * int(len(cand)), "rows_equal": bool(equal)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--one-query-candidates", type=int, default=1_000_000)
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    base = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                            summary_energy=0.5, max_fraction=6.0,
                                                                            use_device=1))
    q = _native.synth(a.queries, a.dim, 43, 1, docs)
    del docs
    n_docs = int(base.desc.n_docs)
    out = {"docs": n_docs, "dim": a.dim, "warmup": WARMUP, "timed": TIMED, "rows": []}
    for vt, vname in ((0, "f16"), (2, "dotvbyte")):
        ix = base if vt == 0 else base.convert(vt)
        ix.upload(0)
        rng = np.random.default_rng(7)
        per = 100
        cand_off = np.arange(a.queries + 1, dtype=np.uint64) * np.uint64(per)
        uniform = rng.integers(0, n_docs, a.queries * per).astype(np.uint64)
        _, ids, n = ix.batch_search(q[0], q[1], q[2], 10, 4, 1.0, False)
        mixed = rng.integers(0, n_docs, (a.queries, per)).astype(np.uint64)
        for i in range(a.queries):
            mixed[i, :n[i]] = ids[i, :n[i]]
        one = (q[0][:2].copy(), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
        one_cand = rng.integers(0, n_docs, a.one_query_candidates).astype(np.uint64)
        one_off = np.array([0, len(one_cand)], np.uint64)
        for name, qq, off, cand, k in (("uniform", q, cand_off, uniform, 10), ("search", q, cand_off, mixed.ravel(), 10),
                                       ("search", q, cand_off, mixed.ravel(), 100), ("one_query", one, one_off, one_cand, 10),
                                       ("one_query", one, one_off, one_cand, 1000)):
            r = measure(ix, name, qq, off, cand, k)
            r["value_type"] = vname
            out["rows"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
