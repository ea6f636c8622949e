#!/usr/bin/env python3
"""sgpu_score_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index. Three workloads:
  uniform   --queries queries x 100 candidates drawn uniformly
  search    --queries queries x the ids each query's own search returns (k = 10, query_cut 4, heap_factor 1.0) plus
            random ids up to 100
  one_query 1 query x 1 000 000 candidates drawn uniformly
Per workload, after 3 warm-up calls, 20 timed calls; one JSON line with
  kernel_ms        device time of a call's kernels (HIP events inside the launcher: sgpu_debug_score_stats), median
  call_ms          the call from host buffers to host scores (wall clock), median
  cand_per_s       candidates / kernel time
  algo_bytes       record bytes + 8 B ref + 8 B id + 4 B score per candidate, + the queries (8 B per component, 8 B per
                   offset); record bytes are the stored records' (padded to 8 elements; DotVByte: 20 B per slice, raw
                   form 3 B per element), taken from a sample of at most 100 000 of the call's candidates
  frac_of_peak     algo_bytes / kernel time over PEAK_GBS
The ceiling of this access pattern is not the streaming rate: a candidate's record is about four scattered 128-byte
lines (tools/ubench/random_record_read.hip, profiles/r02_ubench_random_record_read.txt: 4.5 - 4.8 TB/s useful for 480-byte
records at 16-byte alignment from an 8 GB buffer).

  python tools/score_probe.py > profiles/score_documents.json
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

PEAK_GBS = 8000.0
WARMUP, TIMED = 3, 20


def stats(ix):
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(8, np.float64)
    _native.check(L.sgpu_debug_score_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return out


def record_bytes(ix, cand, rng):
    """Mean stored bytes of the candidates' records, from a sample."""
    d = ix.desc
    off = np.ctypeslib.as_array(C.cast(C.c_void_p(d.fwd_offsets) if isinstance(d.fwd_offsets, int) else d.fwd_offsets, C.POINTER(C.c_uint64)),
                                (int(d.n_docs) + 1,))
    sample = cand if len(cand) <= 100_000 else rng.choice(cand, 100_000, replace=False)
    lens = (off[sample + 1] - off[sample]).astype(np.int64)
    npad = (lens + 7) & ~7
    if d.value_type == 0:
        return float((npad * (d.comp_width + 2)).mean())
    if d.value_type == 1:
        return float((npad * (d.comp_width + 1)).mean())
    comps = np.ctypeslib.as_array(C.cast(C.c_void_p(d.fwd_comps), C.POINTER(C.c_uint16)), (int(d.nnz),))
    total = 0
    for s, n, p in zip(off[sample].astype(np.int64), lens, npad):   # (the raw form: a gap that does not fit its field)
        c = comps[s:s + n].astype(np.int64)
        gaps = np.diff(c)
        pos = np.arange(1, n)
        limit = np.where((pos & 7) <= 3, 4096, 2048)
        raw = bool(np.any((gaps >= limit) & ((pos & 7) != 0))) if n > 1 else False
        total += p * 3 if raw else p // 8 * 20
    return total / len(sample)


def measure(ix, name, q, cand_off, cand, rng):
    nq = len(q[0]) - 1
    kernel, wall, st = [], [], None
    for i in range(WARMUP + TIMED):
        t = time.perf_counter()
        ix.score_documents(q[0], q[1], q[2], cand_off, cand)
        w = (time.perf_counter() - t) * 1e3
        st = stats(ix)
        if i >= WARMUP:
            kernel.append(st[0])
            wall.append(w)
    k_ms, c_ms = float(np.median(kernel)), float(np.median(wall))
    rec = record_bytes(ix, cand.astype(np.int64), rng)
    algo = len(cand) * (rec + 20.0) + 8.0 * len(q[1]) + 8.0 * (nq + 1)
    return {"workload": name, "queries": nq, "candidates": int(len(cand)), "launches": int(st[1]),
            "lookup": "dense" if st[2] else "hash", "grid": int(st[3]), "block": int(st[4]), "lds_bytes": int(st[5]),
            "kernel_ms": round(k_ms, 4), "kernel_ms_min": round(float(np.min(kernel)), 4),
            "kernel_ms_max": round(float(np.max(kernel)), 4), "call_ms": round(c_ms, 3),
            "cand_per_s": round(len(cand) / (k_ms * 1e-3)), "record_bytes_mean": round(rec, 1),
            "algo_bytes": int(algo), "algo_gbs": round(algo / (k_ms * 1e6), 1),
            "frac_of_peak": round(algo / (k_ms * 1e6) / PEAK_GBS, 4)}


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
    out = {"docs": n_docs, "dim": a.dim, "peak_gbs": PEAK_GBS, "warmup": WARMUP, "timed": TIMED,
           "gather_ceiling": "profiles/r02_ubench_random_record_read.txt: 4.5 - 4.8 TB/s useful (480 B records, 16 B "
                             "alignment, 8 GB buffer); random 128-byte-line gathers, not streaming, bound this call",
           "rows": []}
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
        for name, qq, off, cand in (("uniform", q, cand_off, uniform), ("search", q, cand_off, mixed.ravel()),
                                    ("one_query", one, np.array([0, len(one_cand)], np.uint64), one_cand)):
            r = measure(ix, name, qq, off, cand, rng)
            r["value_type"] = vname
            out["rows"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
