#!/usr/bin/env python3
"""Exact top-k on the device against the host, on the bench collection (8.8M documents x 30K vocabulary, seed 42;
queries seed 43). Builds a forward-only index the way SeismicDataset._freeze does, uploads it, times the one-time
exact-file build, then device exact for --queries queries at k = 10 and k = 100 (median of 3 calls, host clock
around the synchronous call) and host exact on the first --host-queries of them (--threads threads), asserts
that those rows are identical, and prints one JSON line.

Algorithmic bytes per query: 4 bytes per entry the query's components touch (their document frequencies), plus
the two u32 offsets per (component, range) and the candidates (8 bytes per (range, slot), written and read once).

  python tools/exact_probe.py > profiles/exact_device_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

PEAK_GBS = 8000.0
RANGE = 32768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--host-queries", type=int, default=500)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    df = np.bincount(docs[1], minlength=a.dim).astype(np.int64)
    t = time.perf_counter()
    ix = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=1, centroid_fraction=1.0,
                                                                          min_cluster_size=0, summary_energy=1.0,
                                                                          max_fraction=1.0, doc_cut=1))
    build_s = time.perf_counter() - t
    t = time.perf_counter()
    ix.upload(0)
    upload_s = time.perf_counter() - t
    q = _native.synth(a.queries, a.dim, 43, 1, docs)
    del docs
    one = (q[0][:2].copy(), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
    t = time.perf_counter()
    ix.exact_search_device(*one, 10)   # the first call builds the exact file
    file_s = time.perf_counter() - t

    n_ranges = (a.docs + RANGE - 1) // RANGE
    qo = q[0].astype(np.int64)
    qlen = np.diff(qo)
    csum = np.concatenate([[0], np.cumsum(df[q[1]])])
    entries = csum[qo[1:]] - csum[qo[:-1]]
    out = {"docs": a.docs, "dim": a.dim, "queries": a.queries, "build_forward_index_s": round(build_s, 2),
           "upload_s": round(upload_s, 2), "exact_file_build_s": round(file_s, 3),
           "entries_touched_per_query": round(float(entries.mean()), 1)}
    hn = a.host_queries
    hq = (q[0][:hn + 1].copy(), q[1][:int(q[0][hn])], q[2][:int(q[0][hn])])
    for k in (10, 100):
        times, res = [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            res = ix.exact_search_device(*q, k)
            times.append(time.perf_counter() - t)
        dev_s = float(np.median(times))
        t = time.perf_counter()
        host = ix.exact_search(*hq, k, a.threads)
        host_s = time.perf_counter() - t
        same = (np.array_equal(res[2][:hn], host[2]) and np.array_equal(res[1][:hn], host[1])
                and np.array_equal(res[0][:hn].view(np.uint32), host[0].view(np.uint32)))
        assert same, "device and host exact differ at k=%d" % k
        bytes_q = float((entries * 4).mean() + qlen.mean() * n_ranges * 8 + n_ranges * k * 8 * 2)
        dev_ms = dev_s * 1e3 / a.queries
        host_ms = host_s * 1e3 / hn
        gbs = bytes_q * a.queries / dev_s / 1e9
        out["k%d" % k] = {"device_s": round(dev_s, 4), "device_ms_per_query": round(dev_ms, 5),
                          "host_ms_per_query": round(host_ms, 3), "speedup": round(host_ms / dev_ms, 1),
                          "identical_on_host_queries": hn, "bytes_per_query": round(bytes_q),
                          "achieved_GBs": round(gbs, 1), "share_of_8TBs": round(gbs / PEAK_GBS, 3),
                          "device_calls_s": [round(x, 4) for x in times]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
