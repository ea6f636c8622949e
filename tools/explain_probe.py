#!/usr/bin/env python3
"""sgpu_explain_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index: --queries queries x 100 and x 10 candidates drawn uniformly, m = 10
and m = 32. Per shape, after 3 warm-up calls, 20 timed calls of sgpu_explain_documents and, in the same process and state
and on the same pairs, of sgpu_score_documents; one row with the medians of
  kernel_ms   device time of a call's kernels (HIP events inside the launcher: sgpu_debug_score_stats)
  call_ms     the call from host buffers to host outputs (wall clock)
for both calls and the explain call's ratios to the score call's. The explain kernel does strictly more work per candidate
and the call copies 16 m + 8 bytes back per candidate instead of 4.

  python tools/explain_probe.py > profiles/explain_documents.json
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


def timed(ix, call):
    kernel, wall, st = [], [], None
    for i in range(WARMUP + TIMED):
        t = time.perf_counter()
        call()
        w = (time.perf_counter() - t) * 1e3
        st = stats(ix)
        if i >= WARMUP:
            kernel.append(st[0])
            wall.append(w)
    return float(np.median(kernel)), float(np.median(wall)), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
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
        for per in (100, 10):
            cand_off = np.arange(a.queries + 1, dtype=np.uint64) * np.uint64(per)
            cand = rng.integers(0, n_docs, a.queries * per).astype(np.uint64)
            sk, sc, _ = timed(ix, lambda: ix.score_documents(q[0], q[1], q[2], cand_off, cand))
            for m in (10, 32):
                xk, xc, st = timed(ix, lambda: ix.explain_documents(q[0], q[1], q[2], cand_off, cand, m))
                n_terms = ix.explain_documents(q[0], q[1], q[2], cand_off, cand, m)[1]
                r = {"value_type": vname, "queries": a.queries, "candidates": int(len(cand)), "m": m,
                     "launches": int(st[1]), "lookup": "dense" if st[2] else "hash", "grid": int(st[3]), "block": int(st[4]),
                     "lds_bytes": int(st[5]), "terms_mean": round(float(n_terms.mean()), 2),
                     "explain_kernel_ms": round(xk, 4), "explain_call_ms": round(xc, 3),
                     "score_kernel_ms": round(sk, 4), "score_call_ms": round(sc, 3),
                     "kernel_ratio": round(xk / sk, 2), "call_ratio": round(xc / sc, 2)}
                out["rows"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
