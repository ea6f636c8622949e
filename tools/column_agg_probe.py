#!/usr/bin/env python3
"""Column aggregations on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters) and
the column set of tools/column_probe.py (tenant, category, price f32, ts i32): one JSON line with sgpu_column_stats,
sgpu_column_histogram and sgpu_column_top timed against their alternatives.

Per case -
  device_ms   the device call, wall clock around it (the filter's words up, the kernels, the result down)
  kernel_ms   its kernels, from HIP events (sgpu_debug_column_agg_stats); kernel_bytes = the algorithmic bytes (4 n_docs of
              the column + n_docs / 8 of the filter's words when there is a filter; the top call reads them once per select
              pass, once to count the equals and once to emit: 6 x), kernel_gbps = kernel_bytes / kernel_ms and
              ceiling_fraction = that over the 6.38 TB/s streaming ceiling of profiles/r02_ubench_record_stream.txt
  host_ms     the host twin with --threads threads
  numpy_ms    what a user does today: get_column + the filter's get_bits + np.min / max / sum, np.histogram, or
              np.argpartition + a sort of the cut
  winner      the fastest of device_ms, host_ms and numpy_ms
Cases: stats of price over all documents and the 50 % filter; histograms of price into 20 buckets and of ts into 4096
buckets over both; top of ts at t = 10 and t = 1000 in both orders over all documents and the 0.1 % filter.
Medians of --reps timed calls after --warmup. The device results are checked against the host twins'.

  python tools/column_agg_probe.py > profiles/column_aggregations.json
"""
import argparse
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

TENANT, CATEGORY, PRICE, TS = 0, 1, 2, 3
CEILING_GBPS = 6380.0


def timed(fn, warmup, reps):
    """(median wall ms of the timed calls, the last result, what `fn` returned beside it per timed call)"""
    ms, extra, res = [], [], None
    for i in range(warmup + reps):
        t = time.perf_counter()
        res, x = fn()
        dt = (time.perf_counter() - t) * 1e3
        if i >= warmup:
            ms.append(dt)
            extra.append(x)
    return float(np.median(ms)), res, extra


def unpack(flt, n):
    return np.unpackbits(flt.bits().view(np.uint8), bitorder="little")[:n].astype(bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="what to record as the commit when the tree is not a git checkout")
    ap.add_argument("--parent", default=None, help="recorded as parent_commit: the commit the measured tree was made on")
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
    for slot, col in cols.items():
        ix.set_column(slot, col)
    ix.upload(0)
    half = ix.make_filter(cols[PRICE] <= 50.0)
    tiny = ix.make_filter((cols[TS] >= 0) & (cols[TS] <= year // 1000))
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = a.commit
    out = {"docs": n, "dim": a.dim, "warmup": a.warmup, "reps": a.reps, "host_threads": a.threads, "commit": commit, "parent_commit": a.parent,
           "library": _native.build_info(), "streaming_ceiling": "6.38 TB/s (profiles/r02_ubench_record_stream.txt)", "cases": []}

    def record(call, case, fname, flt, dev_fn, host_fn, numpy_fn, hook_key, same, passes_read=1):
        dev_ms, dev, ker = timed(lambda: (dev_fn(), ix.debug_column_agg_stats()), a.warmup, a.reps)
        host_ms, host, _ = timed(lambda: (host_fn(), None), 1, a.host_reps)
        numpy_ms, ref, _ = timed(lambda: (numpy_fn(), None), 0, 3)
        kernel_ms = float(np.median([k[hook_key + "_ms"] for k in ker]))
        kbytes = passes_read * (4 * n + (n // 8 if flt is not None else 0))
        gbps = kbytes / kernel_ms / 1e6
        times = {"device": dev_ms, "host": host_ms, "numpy": numpy_ms}
        r = {"call": call, "case": case, "filter": fname, "docs": n if flt is None else flt.count, "grid": ker[-1][hook_key + "_grid"],
             "device_ms": round(dev_ms, 4), "kernel_ms": round(kernel_ms, 4), "kernel_bytes": kbytes, "kernel_gbps": round(gbps, 1),
             "ceiling_fraction": round(gbps / CEILING_GBPS, 4), "host_ms": round(host_ms, 3), "numpy_ms": round(numpy_ms, 2),
             "winner": min(times, key=times.get), "device_equals_host": bool(same(dev, host)), "numpy_agrees": bool(same(dev, ref, True))}
        if call == "top":
            r["select_passes"] = ker[-1]["top_passes"]
        out["cases"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)

    # ---- stats: price
    def same_stats(x, y, loose=False):
        if loose:        # numpy sums pairwise in another order: the order-free fields, and the sum to 1e-9 relative
            return (x["docs"], x["valid"], x["min_bits"], x["max_bits"]) == y[:4] and abs(x["sum"] - y[4]) <= 1e-9 * abs(y[4])
        return x == y
    for fname, flt in (("all", None), ("range_50pct", half)):
        def numpy_stats():
            v = ix.get_column(PRICE)
            if flt is not None:
                v = v[unpack(flt, n)]
            ok = v[~np.isnan(v)]
            return (len(v), len(ok), int(np.array([ok.min() + np.float32(0)]).view(np.uint32)[0]),
                    int(np.array([ok.max() + np.float32(0)]).view(np.uint32)[0]), float(ok.sum(dtype=np.float64)))
        record("stats", "price", fname, flt, lambda: ix.column_stats(PRICE, flt), lambda: ix.column_stats(PRICE, flt, host=True, num_threads=a.threads),
               numpy_stats, "stats", same_stats)

    # ---- histogram: price into 20 buckets, ts into 4096
    def same_hist(x, y, loose=False):
        return np.array_equal(x[0], y[0]) and (loose or tuple(x[1:]) == tuple(y[1:]))
    hists = (("price_20_buckets", PRICE, np.linspace(0, 100, 21).astype(np.float32)),
             ("ts_4096_buckets", TS, np.linspace(-year // 2, year // 2, 4097).astype(np.int64).astype(np.int32)))
    for case, slot, edges in hists:
        for fname, flt in (("all", None), ("range_50pct", half)):
            def numpy_hist():
                v = ix.get_column(slot)
                if flt is not None:
                    v = v[unpack(flt, n)]
                return (np.histogram(v, edges)[0].astype(np.uint64),)
            eb = edges.view(np.uint32)
            record("histogram", case, fname, flt, lambda: ix.column_histogram(slot, eb, flt),
                   lambda: ix.column_histogram(slot, eb, flt, host=True, num_threads=a.threads), numpy_hist, "hist", same_hist)

    # ---- top: ts at t = 10 and t = 1000, both orders
    def same_top(x, y, loose=False):
        return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and (loose or tuple(x[2:]) == tuple(y[2:]))
    for top in (10, 1000):
        for order in (0, 1):
            for fname, flt in (("all", None), ("range_0.1pct", tiny)):
                def numpy_top():
                    v = ix.get_column(TS)
                    ids = np.arange(n) if flt is None else np.flatnonzero(unpack(flt, n))
                    key = v[ids].astype(np.int64)
                    key = (-key if order else key) * (1 << 32) + ids      # (value, id) as one key: ties by id ascending
                    cut = np.argpartition(key, top - 1)[:top] if len(key) > top else np.arange(len(key))
                    rows = ids[cut[np.argsort(key[cut])]]
                    return rows.astype(np.uint32), v.view(np.uint32)[rows]
                record("top", "ts_t%d_%s" % (top, "desc" if order else "asc"), fname, flt, lambda: ix.column_top(TS, top, order, flt),
                       lambda: ix.column_top(TS, top, order, flt, host=True, num_threads=a.threads), numpy_top, "top", same_top,
                       passes_read=6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
