#!/usr/bin/env python3
"""Term filters on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters), as an f16
and as a DotVByte index: one JSON line with, per index and clause set,
  device_ms   sgpu_filter_create_terms, wall clock around the call (clauses up, kernel, words and count down)
  kernel_ms   its one kernel, from HIP events (sgpu_debug_term_filter_stats)
  host_ms     sgpu_filter_create_terms_host with --threads threads on the same box
  numpy_ms    the scan over get_desc()'s forward arrays a user would write without the call (one timed run; null for
              the 1024 clauses: a pass over the collection per clause)
  count       matching documents; the device words are checked against the host twin's
medians of --reps timed calls after --warmup, and the one-off cost of the exact file's build (wall ms, bytes).
Clause sets: one MUST on the most frequent component, one MUST on a rare one, 8 SHOULD with min_should = 2, 1024 clauses.

  python tools/term_filter_probe.py > profiles/term_filter.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_term_filter_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

MUST, MUST_NOT, SHOULD = 0, 1, 2
NINF = float("-inf")


def stats(ix):
    L = _native.lib()
    L.sgpu_debug_term_filter_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(4, np.float64)
    _native.check(L.sgpu_debug_term_filter_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return out


def numpy_scan(d, clauses, min_should):
    """What a user writes today: a pass over the forward arrays per clause."""
    n_docs, nnz = int(d.n_docs), int(d.nnz)
    off = np.ctypeslib.as_array(d.fwd_offsets, (n_docs + 1,))
    comps = np.ctypeslib.as_array(C.cast(d.fwd_comps, C.POINTER(C.c_uint16 if d.comp_width == 2 else C.c_uint32)), (nnz,))
    f16 = int(d.value_type) == 0
    raw = np.ctypeslib.as_array(C.cast(d.fwd_vals, C.POINTER(C.c_uint16 if f16 else C.c_uint8)), (nnz,))
    n_must = sum(1 for _, o, _ in clauses if o == MUST)
    must, should, banned = np.zeros(n_docs, np.int32), np.zeros(n_docs, np.int32), np.zeros(n_docs, bool)
    for c, occur, mw in clauses:
        ent = np.flatnonzero(comps == c)
        v = raw[ent].view(np.float16).astype(np.float32) if f16 else raw[ent].astype(np.float32) * np.float32(d.val_scale)
        hit = np.searchsorted(off, ent[v >= np.float32(mw)], side="right") - 1
        if occur == MUST:
            must[hit] += 1
        elif occur == SHOULD:
            should[hit] += 1
        else:
            banned[hit] = True
    return (must == n_must) & ~banned & (should >= min_should)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--numpy-max-clauses", type=int, default=8,
                    help="the numpy scan is timed for clause sets up to this size (it costs a pass over the collection per clause)")
    ap.add_argument("--commit", default=None, help="what to record as the commit when the tree is not a git checkout")
    a = ap.parse_args()

    docs = _native.synth(a.docs, a.dim, 42, 0)
    base = _native.NativeIndex.build(2, a.dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                            summary_energy=0.5, max_fraction=6.0, use_device=1))
    del docs
    d = base.desc
    n_docs, nnz = int(d.n_docs), int(d.nnz)
    freq = np.bincount(np.ctypeslib.as_array(C.cast(d.fwd_comps, C.POINTER(C.c_uint16)), (nnz,)), minlength=a.dim)
    by_freq = np.argsort(-freq, kind="stable")
    stored = by_freq[freq[by_freq] > 0]
    rare = int(stored[-max(len(stored) // 10, 1)])               # a component of the rarest tenth that is stored at all
    rng = np.random.default_rng(11)
    many = [(int(c), SHOULD, float(w)) for c, w in zip(rng.choice(stored[:4096], 1000), rng.random(1000))]
    many += [(int(by_freq[0]), MUST, NINF)] * 8 + [(int(c), MUST_NOT, 1.0) for c in rng.choice(stored[:4096], 16)]
    sets = [("must_frequent", [(int(by_freq[0]), MUST, NINF)], 0), ("must_rare", [(rare, MUST, NINF)], 0),
            ("should8_min2", [(int(c), SHOULD, NINF) for c in by_freq[8:16]], 2), ("clauses_1024", many, 20)]
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = a.commit
    out = {"docs": n_docs, "dim": a.dim, "nnz": nnz, "warmup": a.warmup, "reps": a.reps, "host_threads": a.threads,
           "commit": commit, "library": _native.build_info(), "indexes": []}
    for kind, ix in (("f16", base), ("dotvbyte", base.convert(2))):
        ix.upload(0)
        t = time.perf_counter()
        ix.make_term_filter(sets[0][1], 0).close()               # the first call on the replica: builds the exact file
        first_ms = (time.perf_counter() - t) * 1e3
        s = stats(ix)
        rows = []
        for name, clauses, ms in sets:
            cl = _native.term_clauses(clauses)
            dev, ker, host = [], [], []
            for i in range(a.warmup + a.reps):
                t = time.perf_counter()
                f = ix.make_term_filter(cl, ms)
                dt = (time.perf_counter() - t) * 1e3
                if i >= a.warmup:
                    dev.append(dt)
                    ker.append(float(stats(ix)[0]))
                if i + 1 < a.warmup + a.reps:
                    f.close()
            few = len(clauses) > 64                              # (the host scan grows with the clauses: one timed call, no warm-up)
            for i in range(1 if few else 1 + min(a.reps, 5)):
                t = time.perf_counter()
                h = ix.make_term_filter(cl, ms, host=True, num_threads=a.threads)
                if i or few:
                    host.append((time.perf_counter() - t) * 1e3)
                same = bool(np.array_equal(h.bits(), f.bits())) and h.count == f.count
                h.close()
            numpy_ms, ok = None, None
            if len(clauses) <= a.numpy_max_clauses:              # (a pass over all stored components per clause)
                t = time.perf_counter()
                ok = numpy_scan(ix.desc, clauses, ms)
                numpy_ms = round((time.perf_counter() - t) * 1e3, 1)
            r = {"clauses": name, "n_clauses": len(clauses), "min_should": ms, "count": f.count,
                 "segment_bytes": int(4 * sum(int(freq[c]) for c, _, _ in clauses)),
                 "device_ms": round(float(np.median(dev)), 4), "kernel_ms": round(float(np.median(ker)), 4),
                 "host_ms": round(float(np.median(host)), 3), "host_timed_calls": len(host), "numpy_ms": numpy_ms,
                 "device_equals_host": same, "numpy_equals_device": None if ok is None else bool(int(ok.sum()) == f.count)}
            f.close()
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        out["indexes"].append({"value_type": kind, "first_call_ms": round(first_ms, 1), "exact_file_build_wall_ms": round(float(s[1]), 1),
                               "exact_file_bytes": int(s[2]), "ranges": int(s[3]), "clause_sets": rows})
        ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
