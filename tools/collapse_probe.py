#!/usr/bin/env python3
"""sgpu_collapse_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index. Shapes: --queries queries x 100 candidates (their own search
results, filled up with random ids), four consecutive document ids per group, k = 10 at m = 1 and m = 3; the same queries
x 1000 candidates at k = 10; one query x 4096. Per shape, after 3 warm-up calls, 20 timed calls; one row with the medians of
  score_kernel_ms, select_ms   device time of the call's score kernels and of its selection kernels (HIP events inside the
                  launcher: sgpu_debug_collapse_stats)
  call_ms         the call from host buffers to host rows (wall clock)
  rerank_select_ms, rerank_call_ms   sgpu_rerank_documents on the same candidates at the same k: what a one-key selection costs
  numpy_lexsort_ms   what a user does without the call: sgpu_score_documents, then the grouping of the whole batch with
                  np.lexsort (distinct pairs, members best first, the first m summed, the k best groups per query)
  numpy_loop_ms   the same as a per-query Python loop (over --python-queries queries, scaled to the batch)
The rows of the device call are checked against the host twin's before timing, the lexsort version's groups against them.

  python tools/collapse_probe.py > profiles/collapse_documents.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_collapse_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

WARMUP, TIMED = 3, 20
PER_GROUP = 4


def score_stats(ix):
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(8, np.float64)
    _native.check(L.sgpu_debug_score_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return out


def numpy_lexsort(ix, q, cand_off, cand, grp, m, k):
    """score_documents, then the whole batch grouped with lexsort -> (group keys [nq, k], counts)."""
    nq = len(cand_off) - 1
    sc = ix.score_documents(q[0], q[1], q[2], cand_off, cand)
    qid = np.repeat(np.arange(nq), np.diff(cand_off.astype(np.int64)))
    o = np.lexsort((cand, -sc.astype(np.float64), grp, qid))   # query, group, score descending, id
    qs, gs, ids, ss = qid[o], grp[o], cand[o], sc[o]
    keep = np.ones(len(o), bool)   # a pair's listings are neighbours (one id, one score): the first of each stays
    keep[1:] = (qs[1:] != qs[:-1]) | (gs[1:] != gs[:-1]) | (ids[1:] != ids[:-1])
    qs, gs, ss = qs[keep], gs[keep], ss[keep]
    head = np.ones(len(qs), bool)
    head[1:] = (qs[1:] != qs[:-1]) | (gs[1:] != gs[:-1])
    start = np.flatnonzero(head)
    rank = np.arange(len(qs)) - np.repeat(start, np.diff(np.append(start, len(qs))))
    total = np.add.reduceat(np.where(rank < m, ss, np.float32(0.0)), start)   # (numpy's own order of additions)
    gq, gk = qs[start], gs[start]
    o2 = np.lexsort((gk, -total.astype(np.float64), gq))
    gq, gk = gq[o2], gk[o2]
    first = np.flatnonzero(np.append(True, gq[1:] != gq[:-1]))
    pos = np.arange(len(gq)) - np.repeat(first, np.diff(np.append(first, len(gq))))
    rows = np.zeros((nq, k), np.uint32)
    sel = pos < k
    rows[gq[sel], pos[sel]] = gk[sel]
    return rows, np.bincount(gq[sel], minlength=nq)


def numpy_loop(ix, q, cand_off, cand, grp, m, k, n):
    """score_documents, then the first n queries grouped one by one: seconds."""
    t0 = time.perf_counter()
    sc = ix.score_documents(q[0], q[1], q[2], cand_off, cand)
    t_score = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(n):
        a, b = int(cand_off[i]), int(cand_off[i + 1])
        best = {}
        for g, d, s in zip(grp[a:b].tolist(), cand[a:b].tolist(), sc[a:b].tolist()):
            best.setdefault(g, {})[d] = s
        rows = []
        for g, mem in best.items():
            top = sorted(mem.items(), key=lambda x: (-x[1], x[0]))
            total = np.float32(top[0][1])
            for _, s in top[1:m]:
                total = np.float32(total + np.float32(s))
            rows.append((g, total, top[0][0], top[0][1], len(top)))
        rows.sort(key=lambda r: (-r[1], r[0]))
        del rows[k:]
    return t_score, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--python-queries", type=int, default=200)
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    print("documents generated", file=sys.stderr, flush=True)
    base = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                            summary_energy=0.5, max_fraction=6.0,
                                                                            use_device=1))
    q = _native.synth(a.queries, a.dim, 43, 1, docs)
    del docs
    print("index built", file=sys.stderr, flush=True)
    n_docs = int(base.desc.n_docs)
    out = {"docs": n_docs, "dim": a.dim, "warmup": WARMUP, "timed": TIMED, "documents_per_group": PER_GROUP, "rows": []}
    rng = np.random.default_rng(7)
    for vt, vname in ((0, "f16"), (2, "dotvbyte")):
        ix = base if vt == 0 else base.convert(vt)
        ix.upload(0)
        print("%s index uploaded" % vname, file=sys.stderr, flush=True)
        sc, ids, n = ix.batch_search(q[0], q[1], q[2], 100, 4, 0.8)

        def filled(width):
            lists = [np.concatenate([ids[i, :n[i]], rng.integers(0, n_docs, width - int(n[i])).astype(np.uint64)])
                     for i in range(a.queries)]
            return np.arange(a.queries + 1, dtype=np.uint64) * width, np.concatenate(lists).astype(np.uint64)

        off100, cand100 = filled(100)
        off1000, cand1000 = filled(1000)
        one_q = (np.array([0, q[0][1]], np.uint64), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
        one = np.concatenate([cand100[:100], rng.integers(0, n_docs, 3996).astype(np.uint64)])
        shapes = [("100", q, off100, cand100, 1, 10), ("100", q, off100, cand100, 3, 10), ("1000", q, off1000, cand1000, 1, 10),
                  ("one", one_q, np.array([0, 4096], np.uint64), one, 1, 10)]
        for shape, qq, cand_off, cand, m, k in shapes:
            nq = len(qq[0]) - 1
            grp = (cand // PER_GROUP).astype(np.uint32)
            dev = ix.collapse_documents(qq[0], qq[1], qq[2], cand_off, cand, grp, m, k)
            host = ix.collapse_documents_host(qq[0], qq[1], qq[2], cand_off, cand, grp, m, k, num_threads=16)
            same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(dev, host))
            t0 = time.perf_counter()
            lex_rows, lex_n = numpy_lexsort(ix, qq, cand_off, cand, grp, m, k)
            lex_ms = (time.perf_counter() - t0) * 1e3
            # (m = 1 sums nothing: there the lexsort version's groups are the call's, ties in the group score aside)
            lex_equal = float((lex_rows == dev[0]).mean())
            kernel, select, wall, rsel, rwall = [], [], [], [], []
            for i in range(WARMUP + TIMED):
                t0 = time.perf_counter()
                ix.collapse_documents(qq[0], qq[1], qq[2], cand_off, cand, grp, m, k)
                ms = (time.perf_counter() - t0) * 1e3
                st = ix.debug_collapse_stats()
                t0 = time.perf_counter()
                ix.rerank_documents(qq[0], qq[1], qq[2], cand_off, cand, k)
                rms = (time.perf_counter() - t0) * 1e3
                rst = score_stats(ix)
                if i >= WARMUP:
                    kernel.append(st["kernel_ms"])
                    select.append(st["select_ms"])
                    wall.append(ms)
                    rsel.append(float(rst[6]))
                    rwall.append(rms)
            nn = min(a.python_queries, nq)
            t_score, t_loop = numpy_loop(ix, qq, cand_off, cand, grp, m, k, nn)
            loop_ms = (t_score + t_loop * nq / nn) * 1e3
            call = float(np.median(wall))
            r = {"value_type": vname, "shape": shape, "queries": nq, "candidates": int(len(cand)), "m": m, "k": k,
                 "rows_equal_host": bool(same), "groups_mean": round(float(dev[5].mean()), 1), "launches": st["launches"],
                 "select_launches": st["select_launches"], "table": "dense" if st["dense"] else "hash",
                 "score_kernel_ms": round(float(np.median(kernel)), 4), "select_ms": round(float(np.median(select)), 4),
                 "call_ms": round(call, 3), "rerank_select_ms": round(float(np.median(rsel)), 4),
                 "rerank_call_ms": round(float(np.median(rwall)), 3), "numpy_lexsort_ms": round(lex_ms, 1),
                 "numpy_lexsort_groups_equal": round(lex_equal, 4), "numpy_loop_ms": round(loop_ms, 1), "python_queries_timed": nn,
                 "lexsort_over_call": round(lex_ms / call, 1), "loop_over_call": round(loop_ms / call, 1)}
            out["rows"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
