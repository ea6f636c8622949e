#!/usr/bin/env python3
"""sgpu_fuse_documents on the bench collection (8.8M documents x 30K vocabulary, seed 42, the bench build parameters;
queries seed 43), for the f16 and the DotVByte index. Shapes: --queries queries x 100 candidates (their own search
results, filled up with random ids; every second candidate in the other list, its score a seeded normal number) and the
same queries x 1000 candidates, k = 10, for each of the three methods. Per shape and method, after 3 warm-up calls, 20 timed
calls; one row with the medians of
  score_kernel_ms, select_ms   device time of the call's score kernels and of its selection kernels (HIP events inside the
                  launcher: sgpu_debug_fuse_stats)
  call_ms         the call from host buffers to host rows (wall clock)
  collapse_select_ms, collapse_call_ms   the yardstick: sgpu_collapse_documents (m = 1, four documents per group) on the same
                  candidates at the same k, in the same loop on the same device - three sorts of the same size against
                  the fusion's four
The rows of the device call are checked against the host twin's before timing. There is no gate.

  python tools/fuse_probe.py > profiles/fuse_documents.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SGPU_TEST_HOOKS", "1")   # (sgpu_debug_fuse_stats is a test hook)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from seismic_amd import _native  # noqa: E402
from seismic_amd._abi import BuildConfig  # noqa: E402

WARMUP, TIMED = 3, 20
PER_GROUP = 4
METHODS = (("rrf", 1.0, 1.0, 60.0), ("minmax", 0.5, 0.5, 0.0), ("sum", 1.0, 0.5, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--value-types", default="f16,dotvbyte")
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
    out = {"docs": n_docs, "dim": a.dim, "warmup": WARMUP, "timed": TIMED, "present_fraction": 0.5, "rows": []}
    rng = np.random.default_rng(7)
    for vt, vname in ((0, "f16"), (2, "dotvbyte")):
        if vname not in a.value_types.split(","):
            continue
        ix = base if vt == 0 else base.convert(vt)
        ix.upload(0)
        print("%s index uploaded" % vname, file=sys.stderr, flush=True)
        sc, ids, n = ix.batch_search(q[0], q[1], q[2], 100, 4, 0.8)

        def filled(width):
            lists = [np.concatenate([ids[i, :n[i]], rng.integers(0, n_docs, width - int(n[i])).astype(np.uint64)])
                     for i in range(a.queries)]
            cand = np.concatenate(lists).astype(np.uint64)
            ext = rng.normal(0.0, 4.0, len(cand)).astype(np.float32)
            ext[1::2] = np.nan
            return np.arange(a.queries + 1, dtype=np.uint64) * width, cand, ext

        for shape, (cand_off, cand, ext) in (("100", filled(100)), ("1000", filled(1000))):
            grp = (cand // PER_GROUP).astype(np.uint32)
            for method, ws, we, c in METHODS:
                k = 10
                dev = ix.fuse_documents(q[0], q[1], q[2], cand_off, cand, ext, method, ws, we, c, k)
                host = ix.fuse_documents_host(q[0], q[1], q[2], cand_off, cand, ext, method, ws, we, c, k, num_threads=16)
                same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(dev, host))
                kernel, select, wall, csel, cwall = [], [], [], [], []
                for i in range(WARMUP + TIMED):
                    t0 = time.perf_counter()
                    ix.fuse_documents(q[0], q[1], q[2], cand_off, cand, ext, method, ws, we, c, k)
                    ms = (time.perf_counter() - t0) * 1e3
                    st = ix.debug_fuse_stats()
                    t0 = time.perf_counter()
                    ix.collapse_documents(q[0], q[1], q[2], cand_off, cand, grp, 1, k)
                    cms = (time.perf_counter() - t0) * 1e3
                    cst = ix.debug_collapse_stats()
                    if i >= WARMUP:
                        kernel.append(st["kernel_ms"])
                        select.append(st["select_ms"])
                        wall.append(ms)
                        csel.append(cst["select_ms"])
                        cwall.append(cms)
                r = {"value_type": vname, "shape": shape, "queries": a.queries, "candidates": int(len(cand)), "method": method, "k": k,
                     "rows_equal_host": bool(same), "launches": st["launches"], "select_launches": st["select_launches"],
                     "table": "dense" if st["dense"] else "hash", "score_kernel_ms": round(float(np.median(kernel)), 4),
                     "select_ms": round(float(np.median(select)), 4), "select_ms_min_max": [round(min(select), 4), round(max(select), 4)],
                     "call_ms": round(float(np.median(wall)), 3), "collapse_select_ms": round(float(np.median(csel)), 4),
                     "collapse_select_ms_min_max": [round(min(csel), 4), round(max(csel), 4)],
                     "collapse_call_ms": round(float(np.median(cwall)), 3),
                     "select_over_collapse": round(float(np.median(select)) / max(float(np.median(csel)), 1e-9), 2)}
                out["rows"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        if ix is not base:
            ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
