#!/usr/bin/env python3
"""Document filters on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43): for A covering 100 / 50 / 10 / 1 / 0.1 % of the documents (random, seed 7) and one contiguous id
range (the first 10 %), one JSON line with, per filter:
  build_ms_device / build_ms_wall  the view's build on its first use (device events around its copies and kernels /
                                   wall clock with the allocations; sgpu_debug_filter_build_times)
  bound_ms                         the compaction's byte bound at PEAK_GBS: post_doc read once (4 B per posting), the
                                   flag words written and read (2 x 1/8 B per posting), post_ref and post_doc of the kept
                                   postings read and written (2 x 12 B), the block starts read and written (2 x 4 B per
                                   block) and the bitmap (n_docs / 8 B)
  filter_device_bytes, n_postings, kept_postings
  qps                              sgpu_batch_search_filtered, --queries queries per call, k = 10, the bench's
                                   query_cut 4 and heap_factor 1.0 (median of --reps calls after one warm-up)
  recall_at_10                     against sgpu_exact_search_device_filtered over the same queries
and the unfiltered q/s for comparison. --views-only builds the views and exits (the run rocprofv3 profiles).

  python tools/filter_probe.py > profiles/filter_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_filter_build_times is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

PEAK_GBS = 8000.0


def build_times(f):
    import ctypes as C
    L = _native.lib()
    L.sgpu_debug_filter_build_times.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(2, np.float64)
    _native.check(L.sgpu_debug_filter_build_times(f.h, 0, out.ctypes.data_as(C.c_void_p)))
    return float(out[0]), float(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views-only", action="store_true")
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    ix = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                          summary_energy=0.5, max_fraction=6.0,
                                                                          use_device=1))
    ix.upload(0)
    q = _native.synth(a.queries, a.dim, 43, 1, docs)
    del docs
    one = (q[0][:2].copy(), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
    d = ix.desc
    n_docs, n_post, n_blocks = int(d.n_docs), int(d.n_postings), int(d.n_blocks)
    post_doc = np.ctypeslib.as_array(d.post_doc, (n_post,))
    rng = np.random.default_rng(7)
    sets = [("random_%g%%" % (100 * fr), rng.random(n_docs) < fr) for fr in (1.0, 0.5, 0.1, 0.01, 0.001)]
    sets.append(("range_first_10%", np.arange(n_docs) < n_docs // 10))

    def qps(filt):
        ix.batch_search(*q, 10, 4, 1.0, False, filter=filt)   # warm-up (and the view's build)
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            ix.batch_search(*q, 10, 4, 1.0, False, filter=filt)
            ts.append(time.perf_counter() - t)
        return a.queries / float(np.median(ts))

    out = {"docs": n_docs, "dim": a.dim, "n_postings": n_post, "n_blocks": n_blocks, "queries": a.queries, "k": 10,
           "query_cut": 4, "heap_factor": 1.0, "peak_gbs": PEAK_GBS}
    if not a.views_only:
        out["unfiltered_qps"] = round(qps(None))
    rows = []
    for name, allowed in sets:
        f = ix.make_filter(allowed)
        ix.search(one[1], one[2], 10, 4, 1.0, filter=f)      # first use: builds the view on replica 0
        dev_ms, wall_ms = build_times(f)
        kept = int(allowed[post_doc].sum())
        bound = 4 * n_post + 2 * (n_post / 8) + 24 * kept + 8 * (n_blocks + 1) + n_docs / 8
        r = {"filter": name, "allowed": int(allowed.sum()), "kept_postings": kept,
             "build_ms_device": round(dev_ms, 3), "build_ms_wall": round(wall_ms, 3),
             "bound_ms": round(bound / (PEAK_GBS * 1e6), 3), "bound_bytes": int(bound),
             "filter_device_bytes": f.device_bytes()}
        if not a.views_only:
            r["qps"] = round(qps(f))
            _, gi, gn = ix.batch_search(*q, 10, 4, 1.0, False, filter=f)
            _, ei, en = ix.exact_search_device(*q, 10, filter=f)
            hit = sum(len(set(gi[i, :gn[i]].tolist()) & set(ei[i, :en[i]].tolist())) for i in range(a.queries))
            r["recall_at_10"] = round(hit / max(int(en.sum()), 1), 4)
        rows.append(r)
        f.close()
        print(json.dumps(r), file=sys.stderr, flush=True)
    out["filters"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
