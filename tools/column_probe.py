#!/usr/bin/env python3
"""Document columns on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters): one
JSON line with the column filter and the facet counts timed against their alternatives.

Columns: tenant u32 (1000 values), category u32 (200 000 values, Zipf-like: above kFacetLdsBins, below 1 << 22), price f32
(uniform 0 .. 100), ts i32 (uniform over a year of seconds, negative for the first half: the signed order matters).
Per filter shape - one MUST range of about 50 %, one of about 0.1 %, tenant IN (8 values) AND a ts range AND price <= x,
64 clauses -
  device_ms   sgpu_filter_create_columns, wall clock around the call (plan up, kernel, words and count down)
  kernel_ms   its kernel, from HIP events (sgpu_debug_column_stats); kernel_gbps = (4 n_docs per distinct column +
              n_docs / 8 words) / kernel_ms, to set beside the streaming ceiling of profiles/r02_ubench_record_stream.txt
  host_ms     sgpu_filter_create_columns_host with --threads threads
  numpy_ms    what a user does today: the numpy predicate -> np.flatnonzero -> sgpu_filter_create, in this process
Per facet column (tenant: LDS path; category: global path), over all documents and over the 50 % filter -
  device_ms, count_kernel_ms, select_kernel_ms, host_ms, numpy_ms (np.unique(col[mask], return_counts=True) and the sort)
Medians of --reps timed calls after --warmup. The device results are checked against the host twins'.

  python tools/column_probe.py > profiles/columns.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (the debug hooks)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

MUST, MUST_NOT, SHOULD = 0, 1, 2
RANGE, IN = 0, 1
TENANT, CATEGORY, PRICE, TS = 0, 1, 2, 3


def bits(x, dt):
    return [int(b) for b in np.asarray(x, dt).view(np.uint32).ravel()]


def rng_clause(slot, occur, dt, lo, hi):
    b = bits([lo, hi], dt)
    return (slot, occur, RANGE, b[0], b[1], 0, 0)


def facet_kernels(ix):
    fn = _native.lib().sgpu_debug_facet_kernel_ms
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(2, np.float64)
    _native.check(fn(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return float(out[0]), float(out[1])


def timed(fn, warmup, reps):
    """(median wall ms of the timed calls, the last result, what `fn` returned beside it per timed call)"""
    ms, extra, res = [], [], None
    for i in range(warmup + reps):
        if res is not None and hasattr(res, "close"):
            res.close()
        t = time.perf_counter()
        res, x = fn()
        dt = (time.perf_counter() - t) * 1e3
        if i >= warmup:
            ms.append(dt)
            extra.append(x)
    return float(np.median(ms)), res, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="what to record as the commit when the tree is not a git checkout")
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    ix = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                          summary_energy=0.5, max_fraction=6.0, use_device=1))
    del docs
    n = int(ix.desc.n_docs)
    rng = np.random.default_rng(5)
    year = 365 * 86400
    cols = {TENANT: rng.integers(0, 1000, n).astype(np.uint32),
            CATEGORY: np.minimum((200_000 * rng.random(n) ** 3).astype(np.uint32), 199_999),
            PRICE: (rng.random(n) * 100).astype(np.float32),
            TS: rng.integers(-year // 2, year // 2, n).astype(np.int32)}
    cols[CATEGORY][0] = 199_999
    for slot, col in cols.items():
        ix.set_column(slot, col)
    ix.upload(0)
    tenants = [3, 17, 250, 251, 600, 77, 999, 0]
    t0, t1 = -year // 8, year // 4
    shapes = [
        ("range_50pct", [rng_clause(PRICE, MUST, np.float32, 0.0, 50.0)], 0, [], lambda: cols[PRICE] <= 50.0),
        ("range_0.1pct", [rng_clause(TS, MUST, np.int32, 0, year // 1000)], 0, [], lambda: (cols[TS] >= 0) & (cols[TS] <= year // 1000)),
        ("tenant_in8_ts_price", [(TENANT, MUST, IN, 0, 0, 0, 8), rng_clause(TS, MUST, np.int32, t0, t1),
                                 rng_clause(PRICE, MUST, np.float32, -np.inf, 35.0)], 0, tenants,
         lambda: np.isin(cols[TENANT], tenants) & (cols[TS] >= t0) & (cols[TS] <= t1) & (cols[PRICE] <= 35.0)),
    ]
    many, sv = [], rng.integers(0, 1000, 512).astype(np.uint32).tolist()
    for j in range(60):
        slot = (TENANT, PRICE, TS, CATEGORY)[j % 4]
        if slot == TENANT:
            many.append((TENANT, SHOULD, IN, 0, 0, 8 * j, 64))
        elif slot == PRICE:
            lo = float(rng.random() * 90)
            many.append(rng_clause(PRICE, SHOULD, np.float32, lo, lo + 10))
        elif slot == TS:
            lo = int(rng.integers(-year // 2, year // 3))
            many.append(rng_clause(TS, SHOULD, np.int32, lo, lo + year // 6))
        else:
            lo = int(rng.integers(0, 1000))
            many.append(rng_clause(CATEGORY, SHOULD, np.uint32, lo, lo + 5000))
    many += [rng_clause(PRICE, MUST, np.float32, 1.0, 99.0)] * 2 + [rng_clause(TENANT, MUST_NOT, np.uint32, 500, 520), (TENANT, MUST_NOT, IN, 0, 0, 0, 4)]
    shapes.append(("clauses_64", many, 12, sv, None))
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = a.commit
    out = {"docs": n, "dim": a.dim, "warmup": a.warmup, "reps": a.reps, "host_threads": a.threads, "commit": commit,
           "library": _native.build_info(), "streaming_ceiling": "6.38 TB/s (profiles/r02_ubench_record_stream.txt)",
           "column_bytes": None, "filters": [], "facets": []}
    half = None
    for name, clauses, ms, values, predicate in shapes:
        cl, vals = _native.column_clauses(clauses), np.asarray(values, np.uint32)
        dev_ms, f, ker = timed(lambda: (ix.make_column_filter(cl, ms, vals), None), a.warmup, a.reps)
        ker = []
        for _ in range(a.reps):                                   # the kernel time of 20 more calls (the hook holds the last one's)
            ix.make_column_filter(cl, ms, vals).close()
            ker.append(ix.debug_column_stats()["filter_ms"])
        host_ms, h, _ = timed(lambda: (ix.make_column_filter(cl, ms, vals, host=True, num_threads=a.threads), None), 1, a.host_reps)
        same = bool(np.array_equal(h.bits(), f.bits())) and h.count == f.count
        numpy_ms, numpy_same = None, None
        if predicate is not None:
            numpy_ms, g, _ = timed(lambda: (ix.make_filter(np.flatnonzero(predicate())), None), 1, a.host_reps)
            numpy_same = bool(np.array_equal(g.bits(), f.bits()))
            g.close()
        distinct = len({c[0] for c in clauses})
        kernel_ms = float(np.median(ker))
        kbytes = 4 * n * distinct + n // 8
        r = {"shape": name, "n_clauses": len(clauses), "distinct_columns": distinct, "count": f.count, "fraction": round(f.count / n, 5),
             "device_ms": round(dev_ms, 4), "kernel_ms": round(kernel_ms, 4), "kernel_bytes": kbytes,
             "kernel_gbps": round(kbytes / kernel_ms / 1e6, 1), "host_ms": round(host_ms, 3), "numpy_ms": None if numpy_ms is None else round(numpy_ms, 2),
             "device_equals_host": same, "numpy_equals_device": numpy_same}
        out["filters"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        h.close()
        if name == "range_50pct":
            half = f
        else:
            f.close()
    out["column_bytes"] = ix.debug_column_stats()["column_bytes"]
    half_mask = cols[PRICE] <= 50.0
    for cname, slot in (("tenant", TENANT), ("category", CATEGORY)):
        for fname, flt, mask in (("all", None, None), ("range_50pct", half, half_mask)):
            dev_ms, dev, ker = timed(lambda: (ix.facet_counts(slot, flt, 10), facet_kernels(ix)), a.warmup, a.reps)
            host_ms, host, _ = timed(lambda: (ix.facet_counts(slot, flt, 10, host=True, num_threads=a.threads), None), 1, a.host_reps)

            def with_numpy():
                val, cnt = np.unique(cols[slot] if mask is None else cols[slot][mask], return_counts=True)
                order = np.lexsort((val, -cnt.astype(np.int64)))[:10]
                return (val[order], cnt[order]), None
            numpy_ms, ref, _ = timed(with_numpy, 0, 3)
            s = ix.debug_column_stats()
            r = {"column": cname, "bins": int(cols[slot].max()) + 1, "filter": fname, "path": "global" if s["facet_path"] else "lds",
                 "grid": s["facet_grid"], "docs_per_wg": s["facet_docs_per_wg"], "distinct": dev[2], "docs": dev[3],
                 "device_ms": round(dev_ms, 4), "count_kernel_ms": round(float(np.median([k[0] for k in ker])), 4),
                 "select_kernel_ms": round(float(np.median([k[1] for k in ker])), 4), "host_ms": round(host_ms, 3),
                 "numpy_ms": round(numpy_ms, 2),
                 "device_equals_host": bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and dev[2:] == host[2:]),
                 "numpy_equals_device": bool(np.array_equal(ref[0], dev[0]) and np.array_equal(ref[1], dev[1]))}
            out["facets"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
