#!/usr/bin/env python3
"""sgpu_expand_queries on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index: --queries queries with their own top-10 search results as feedback
documents (weight 0.75 / 10), alpha = 1, at t = 64 and t = 1024. Per shape, after 3 warm-up calls, 20 timed calls; one row
with the medians of
  kernel_ms       device time of the call's kernel (HIP events inside the launcher: sgpu_debug_expand_stats)
  call_ms         the call from host buffers to host rows (wall clock)
  host_call_ms    sgpu_expand_queries_host at 16 threads, same process, same inputs (5 timed calls)
  numpy_ms        the per-query Python loop a user would write over get(): rows summed into a dict, terms selected with
                  numpy (once, over --numpy-queries queries, scaled to the batch)
and the ratios of the last two to call_ms. The rows of the device call are checked against the host twin's before timing.

  python tools/expand_probe.py > profiles/expand_queries.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_expand_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import seismic_amd  # noqa: E402
from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

WARMUP, TIMED, HOST_TIMED = 3, 20, 5


def numpy_loop(raw, q, fb, w, t, n):
    """The first n queries expanded in Python over get(): seconds."""
    t0 = time.perf_counter()
    for i in range(n):
        acc = {}
        for c, v in zip(q[1][int(q[0][i]):int(q[0][i + 1])].tolist(), q[2][int(q[0][i]):int(q[0][i + 1])].tolist()):
            acc[c] = v
        for d in fb[i].tolist():
            comps, vals = raw.get(d)
            for c, v in zip(comps, vals):
                acc[c] = acc.get(c, 0.0) + w * v
        c = np.fromiter(acc.keys(), np.int64, len(acc))
        v = np.fromiter(acc.values(), np.float64, len(acc))
        keep = np.flatnonzero(v > 0)
        best = keep[np.lexsort((c[keep], -v[keep]))][:t]
        best = best[np.argsort(c[best])]
        _ = c[best], v[best]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--numpy-queries", type=int, default=500)
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    print("documents generated", file=sys.stderr, flush=True)
    base = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                            summary_energy=0.5, max_fraction=6.0,
                                                                            use_device=1))
    q = _native.synth(a.queries, a.dim, 43, 1, docs)
    del docs
    print("index built", file=sys.stderr, flush=True)
    out = {"docs": int(base.desc.n_docs), "dim": a.dim, "warmup": WARMUP, "timed": TIMED, "host_threads": 16, "rows": []}
    for vt, vname in ((0, "f16"), (2, "dotvbyte")):
        ix = base if vt == 0 else base.convert(vt)
        ix.upload(0)
        print("%s index uploaded" % vname, file=sys.stderr, flush=True)
        sc, ids, n = ix.batch_search(q[0], q[1], q[2], 10, 4, 0.8)
        fb = [ids[i, :n[i]] for i in range(a.queries)]
        cand_off = np.zeros(a.queries + 1, np.uint64)
        cand_off[1:] = np.cumsum(n)
        cand = np.concatenate(fb).astype(np.uint64)
        w = np.float32(0.75 / 10)
        cand_w = np.full(len(cand), w, np.float32)
        raw = seismic_amd.SeismicIndexRaw(ix, upload=False)
        for t in (64, 1024):
            dev = ix.expand_queries(q[0], q[1], q[2], cand_off, cand, cand_w, 1.0, t)
            host = ix.expand_queries_host(q[0], q[1], q[2], cand_off, cand, cand_w, 1.0, t, num_threads=16)
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev, host))
            kernel, wall, hwall = [], [], []
            for i in range(WARMUP + TIMED):
                t0 = time.perf_counter()
                ix.expand_queries(q[0], q[1], q[2], cand_off, cand, cand_w, 1.0, t)
                ms = (time.perf_counter() - t0) * 1e3
                st = ix.debug_expand_stats()
                if i >= WARMUP:
                    kernel.append(st["kernel_ms"])
                    wall.append(ms)
            for i in range(1 + HOST_TIMED):
                t0 = time.perf_counter()
                ix.expand_queries_host(q[0], q[1], q[2], cand_off, cand, cand_w, 1.0, t, num_threads=16)
                if i:
                    hwall.append((time.perf_counter() - t0) * 1e3)
            nn = min(a.numpy_queries, a.queries)
            numpy_ms = numpy_loop(raw, q, fb, float(w), t, nn) * 1e3 * a.queries / nn
            call = float(np.median(wall))
            r = {"value_type": vname, "queries": a.queries, "candidates": int(len(cand)), "t": t, "rows_equal_host": bool(same),
                 "terms_mean": round(float(dev[2].mean()), 1), "launches": st["launches"],
                 "table": "lds" if st["dense"] else "global", "grid": st["grid"], "block": st["block"], "lds_bytes": st["lds"],
                 "kernel_ms": round(float(np.median(kernel)), 4), "call_ms": round(call, 3),
                 "host_call_ms": round(float(np.median(hwall)), 3), "numpy_ms": round(numpy_ms, 1),
                 "numpy_queries_timed": nn, "host_over_call": round(float(np.median(hwall)) / call, 2),
                 "numpy_over_call": round(numpy_ms / call, 1)}
            out["rows"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
