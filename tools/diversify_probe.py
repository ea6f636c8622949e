#!/usr/bin/env python3
"""sgpu_diversify_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build
parameters; queries seed 43), for the f16 and the DotVByte index. Shapes: --queries queries x 100 candidates (their own
search results, filled up with random ids) at k = 10 and k = 100, and one query x 2048 candidates at k = 256 (a single
workgroup by design); lambda = mu = 0.5. Per shape, after 3 warm-up calls, 20 timed calls; one row with the medians of
  kernel_ms       device time of the call's kernel (HIP events inside the launcher: sgpu_debug_diversify_stats)
  call_ms         the call from host buffers to host rows (wall clock)
  score_kernel_ms, score_call_ms   sgpu_score_documents on the same pairs in the same process: the yardstick. The kernel
                  reads each remaining candidate once per round, so k x that is the natural ceiling; kernel_over_k_score is
                  kernel_ms / (rounds x score_kernel_ms)
  host_call_ms    sgpu_diversify_documents_host at 16 threads, same inputs (2 timed calls)
  python_ms       the per-query loop a user would write over get(): candidate-against-candidate dot products in numpy (once,
                  over --python-queries queries, scaled to the batch)
The rows of the device call are checked against the host twin's before timing.

  python tools/diversify_probe.py > profiles/diversify_documents.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_diversify_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seismic_amd  # noqa: E402
from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

WARMUP, TIMED, HOST_TIMED = 3, 20, 2
LAM, MU = 0.5, 0.5


def score_kernel_ms(ix):
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(8, np.float64)
    _native.check(L.sgpu_debug_score_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return float(out[0])


def python_loop(raw, q, cand_off, cand, k, n, dim):
    """The first n queries diversified in Python over get(): seconds."""
    t0 = time.perf_counter()
    for i in range(n):
        qv = np.zeros(dim, np.float32)
        qv[q[1][int(q[0][i]):int(q[0][i + 1])]] = q[2][int(q[0][i]):int(q[0][i + 1])]
        ids = np.unique(cand[int(cand_off[i]):int(cand_off[i + 1])])
        vecs = [raw.get(int(d)) for d in ids.tolist()]
        rel = np.array([np.dot(qv[np.asarray(c, np.int64)], np.asarray(v, np.float32)) for c, v in vecs], np.float32)
        pen = np.zeros(len(ids), np.float32)
        left = np.ones(len(ids), bool)
        for _ in range(min(k, len(ids))):
            mmr = np.where(left, LAM * rel - MU * pen, -np.inf)
            s = int(np.argmax(mmr))
            left[s] = False
            sv = np.zeros(dim, np.float32)
            sv[np.asarray(vecs[s][0], np.int64)] = vecs[s][1]
            for j in np.flatnonzero(left).tolist():
                pen[j] = max(pen[j], float(np.dot(sv[np.asarray(vecs[j][0], np.int64)], np.asarray(vecs[j][1], np.float32))))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--python-queries", type=int, default=20)
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
    out = {"docs": n_docs, "dim": a.dim, "warmup": WARMUP, "timed": TIMED, "host_threads": 16, "lambda": LAM, "mu": MU,
           "rows": []}
    rng = np.random.default_rng(7)
    for vt, vname in ((0, "f16"), (2, "dotvbyte")):
        ix = base if vt == 0 else base.convert(vt)
        ix.upload(0)
        print("%s index uploaded" % vname, file=sys.stderr, flush=True)
        sc, ids, n = ix.batch_search(q[0], q[1], q[2], 100, 4, 0.8)
        lists = [np.concatenate([ids[i, :n[i]], rng.integers(0, n_docs, 100 - int(n[i])).astype(np.uint64)]) for i in range(a.queries)]
        many_off = np.arange(a.queries + 1, dtype=np.uint64) * 100
        many = np.concatenate(lists).astype(np.uint64)
        one_q = (np.array([0, q[0][1]], np.uint64), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
        one = np.concatenate([lists[0], rng.integers(0, n_docs, 1948).astype(np.uint64)])
        raw = seismic_amd.SeismicIndexRaw(ix, upload=False)
        shapes = [("many", q, many_off, many, 10), ("many", q, many_off, many, 100),
                  ("one", one_q, np.array([0, 2048], np.uint64), one, 256)]
        for shape, qq, cand_off, cand, k in shapes:
            nq = len(qq[0]) - 1
            dev = ix.diversify_documents(qq[0], qq[1], qq[2], cand_off, cand, LAM, MU, k)
            hwall = []
            for i in range(1 + HOST_TIMED):
                t0 = time.perf_counter()
                host = ix.diversify_documents_host(qq[0], qq[1], qq[2], cand_off, cand, LAM, MU, k, num_threads=16)
                if i:
                    hwall.append((time.perf_counter() - t0) * 1e3)
            same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(dev, host))
            kernel, wall, skernel, swall = [], [], [], []
            for i in range(WARMUP + TIMED):
                t0 = time.perf_counter()
                ix.diversify_documents(qq[0], qq[1], qq[2], cand_off, cand, LAM, MU, k)
                ms = (time.perf_counter() - t0) * 1e3
                st = ix.debug_diversify_stats()
                t0 = time.perf_counter()
                ix.score_documents(qq[0], qq[1], qq[2], cand_off, cand)
                sms = (time.perf_counter() - t0) * 1e3
                sk_ms = score_kernel_ms(ix)
                if i >= WARMUP:
                    kernel.append(st["kernel_ms"])
                    wall.append(ms)
                    skernel.append(sk_ms)
                    swall.append(sms)
            nn = min(a.python_queries, nq)
            python_ms = python_loop(raw, qq, cand_off, cand, k, nn, a.dim) * 1e3 * nq / nn
            call, kern, sk = float(np.median(wall)), float(np.median(kernel)), float(np.median(skernel))
            r = {"value_type": vname, "shape": shape, "queries": nq, "candidates": int(len(cand)), "k": k,
                 "rows_equal_host": bool(same), "selected_mean": round(float(dev[3].mean()), 1), "rounds": st["rounds"],
                 "launches": st["launches"], "table": "dense" if st["dense"] else "hash", "grid": st["grid"], "block": st["block"],
                 "lds_bytes": st["lds"], "kernel_ms": round(kern, 4), "call_ms": round(call, 3), "score_kernel_ms": round(sk, 4),
                 "score_call_ms": round(float(np.median(swall)), 3), "kernel_over_score": round(kern / sk, 2),
                 "kernel_over_k_score": round(kern / (st["rounds"] * sk), 3), "host_call_ms": round(float(np.median(hwall)), 3),
                 "python_ms": round(python_ms, 1), "python_queries_timed": nn, "host_over_call": round(float(np.median(hwall)) / call, 2),
                 "python_over_call": round(python_ms / call, 1)}
            out["rows"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
