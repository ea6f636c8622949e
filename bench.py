#!/usr/bin/env python3
"""bench.py — Seismic search hot path on MI355X: queries/sec at fixed recall@10.

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): MS MARCO passage /
SPLADE-v3 shape, 8.8M docs x 30K vocab x ~120 nnz/doc, synthetic (SURVEY.md 8d generator), index
parameters of best_configs/msmarco-v1/splade-v3/mem_budget_2.0/recall_95.toml (n_postings=2000,
centroid_fraction=0.2, summary_energy=0.5, max_fraction=6, min_cluster_size=2, doc_cut=15), query
parameters query_cut=4, heap_factor=1.0, first_sorted=false, k=10.

A "step" is ONE call of the drop-in entry point sgpu_batch_search over one batch of 10 000 queries
(BASELINE configs[3]'s batch): host buffers in, host buffers out - validation, launch plan, H2D of the
queries, the search kernel, D2H of the results are all inside the timed region, index
resident in HBM. The K steps are issued by --host-threads request threads (default 2, as a serving
process would: a call returns its rows before the thread issues its next one). Every step of a run
(warm-up included) searches a batch no other step has seen: nothing is cached between steps.
`roofline` stays on the kernel: a second leg launches the same batches device-resident (HIP events on
the library's stream give the kernel duration); its rate is reported as `device_resident`.

  python bench.py --gpus N --steps K --warmup W
N>1 is launched through torch.distributed.run, one rank per GPU, index replicated in every GPU's
HBM, no collective on the data path:
  --scaling strong (default for N>1; BASELINE configs[3]): each 10 000-query batch is cut into N
      contiguous shards, one per GPU; `value` = 10 000 x K / max-over-ranks time.
  --scaling weak: every GPU searches its own 10 000-query batches.

A plain run sets up, warms up, times the K steps and prints the headline (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, the configuration). --full adds everything else the line has
carried: the device-resident kernel leg and its roofline, the counted passes, end-to-end and batch-1 latency,
recall vs exact, the fixed-recall operating points, cpu_baseline and, for N>1, the one-batch-at-a-time,
replica and sharded-identity legs; the --no-* options below skip legs of a --full run.
--dump-outputs DIR writes the rows the timed path returned in its last step (scores.npy f32, ids.npy and
counts.npy f64, rows.npy = their query rows; `_rank<r>` suffixes for N>1).

Real data instead of synthetic: --documents documents.bin --queries-file queries.bin
[--full --groundtruth groundtruth.tsv] [--full --results-tsv out.tsv] (Seismic's inner format and the TSV
of perf_inverted_index).

Prints ONE JSON line on rank 0 (fields: DESIGN.md "Measurement").
"""
import argparse
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 measured achievable
METRIC = "queries/sec + mean latency (µs) at fixed recall@10 vs exact, SPLADE-v3 MSMARCO"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--docs", type=int, default=8_800_000)
    ap.add_argument("--dim", type=int, default=30_000)
    ap.add_argument("--queries", type=int, default=10_000, help="queries per step (one batch)")
    ap.add_argument("--collection", choices=["survey", "clustered"], default="survey",
                    help="synthetic collection: `survey` = the SURVEY 8(d) law (the headline); `clustered` = same sizes, documents "
                         "drawn around latent intents and queries carrying their source document's weights (synth.cpp): work "
                         "per query and recall at the reference's parameters in the range published for MS MARCO")
    ap.add_argument("--batches", type=int, default=0,
                    help="distinct resident batches (0 = one per step incl. warm-up, at most 64)")
    ap.add_argument("--scaling", choices=["auto", "strong", "weak"], default="auto")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--query-cut", type=int, default=4)
    ap.add_argument("--heap-factor", type=float, default=1.0)
    ap.add_argument("--first-sorted", type=int, default=0)
    ap.add_argument("--n-postings", type=int, default=2000)
    ap.add_argument("--centroid-fraction", type=float, default=0.2)
    ap.add_argument("--summary-energy", type=float, default=0.5)
    ap.add_argument("--max-fraction", type=float, default=6.0)
    ap.add_argument("--min-cluster-size", type=int, default=2)
    ap.add_argument("--comp-width", type=int, default=2, choices=[2, 4])
    ap.add_argument("--value-type", default="f16", choices=["f16", "fixedu8", "dotvbyte"],
                    help="forward index storage (fixedu8: u8 fixed-point values; dotvbyte: those plus the compressed "
                         "component stream - the forward index of the reference's DotVByte index)")
    ap.add_argument("--sample", type=int, default=1000,
                    help="queries of the first timed batch used for recall, the oracle identity check and cpu_baseline")
    ap.add_argument("--heldout", type=int, default=4000,
                    help="queries of the same batch, disjoint from --sample, on which every operating point's recall is "
                         "REPORTED (its parameters are selected on the sample only)")
    ap.add_argument("--build-on-host", action="store_true",
                    help="build the index on the host cores only (default: the clustering step runs on the GPU; "
                         "the index is byte-identical either way)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-recall", action="store_true", help="skip recall@k vs exact")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 latency measurement")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end sgpu_batch_search measurement")
    ap.add_argument("--no-weak-leg", action="store_true",
                    help="N>1, strong scaling: skip the extra replicas (weak scaling) measurement")
    ap.add_argument("--all-legs", action="store_true",
                    help="N>1: also run the single-GPU legs (end to end, latency, recall) on rank 0")
    ap.add_argument("--host-threads", type=int, default=0,
                    help="request threads issuing the timed sgpu_batch_search calls (each call is synchronous); 0 = by the "
                         "size of a call: 2 for calls of 2500 queries or more, 3 for smaller ones (one rank's shard of a "
                         "10 000-query batch on 8 GPUs is 1250 queries: profiles/r04_shard_probe.txt)")
    ap.add_argument("--target-recall", default="0.90,0.95,0.99",
                    help="operating points: for each recall@k the cheapest (query_cut, heap_factor, first_sorted) on this "
                         "index that reaches it on the sample (empty string = skip)")
    ap.add_argument("--no-entry", action="store_true",
                    help="profiling runs: skip the entry-point calls, the timed region is the device-resident kernel leg "
                         "(every dispatch of the search kernel is then one whole batch)")
    ap.add_argument("--no-accounting", action="store_true",
                    help="skip the counted passes (PMC profiling runs: only the timed kernel variant is dispatched)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="CPU baseline time budget")
    ap.add_argument("--index-cache", default=os.environ.get("SGPU_INDEX_CACHE", ""))
    ap.add_argument("--traffic-bytes", type=float, default=None,
                    help="HBM bytes per launch measured by a separate rocprofv3 --pmc pass (roofline.traffic)")
    # real data (Seismic's inner binary format / perf_inverted_index TSV)
    ap.add_argument("--documents", default="", help="documents.bin (inner format) instead of synthetic documents")
    ap.add_argument("--queries-file", default="", help="queries.bin (inner format) instead of synthetic queries")
    ap.add_argument("--groundtruth", default="", help="groundtruth.tsv: accuracy as scripts/run_experiments.py computes it")
    ap.add_argument("--results-tsv", default="", help="write query_idx\\tdoc_id\\trank\\tscore of the first batch here")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg besides the timed steps (kernel leg, roofline, latency, recall, operating "
                         "points, cpu_baseline, N>1 legs); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the rows the timed path returned in its last step to DIR/<name>.npy")
    args = ap.parse_args()
    if (args.groundtruth or args.results_tsv) and not args.full:
        ap.error("--groundtruth and --results-tsv belong to a --full run")
    return args


def workload_key(args, world, scaling):
    src = "docs=%d dim=%d" % (args.docs, args.dim) if not args.documents else "documents=%s" % os.path.basename(args.documents)
    if args.collection != "survey" and not args.documents:
        src += " collection=" + args.collection
    key = "%s queries=%d k=%d query_cut=%d heap_factor=%s first_sorted=%d cw=%d np=%d cf=%g se=%g mf=%g" % (
        src, args.queries, args.k, args.query_cut, args.heap_factor, args.first_sorted, args.comp_width,
        args.n_postings, args.centroid_fraction, args.summary_energy, args.max_fraction)
    return key if args.value_type == "f16" else key + " vt=" + args.value_type


def cpu_quota(root="/sys/fs/cgroup"):
    """CPUs' worth of time per accounting period this container may use (cgroup v2 cpu.max, v1 cfs quota); None = no quota."""
    try:
        q, per = open(os.path.join(root, "cpu.max")).read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open(os.path.join(root, "cpu", "cpu.cfs_quota_us")).read())
        per = float(open(os.path.join(root, "cpu", "cpu.cfs_period_us")).read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def kernel_source_id():
    """Identity of the search kernel's source (what a recorded PMC traffic figure belongs to)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "seismic_amd", "csrc")
    for f in ["search_kernel.inc", "device_types.hpp"] + sorted(os.path.basename(x) for x in glob.glob(os.path.join(csrc, "sk_*.hip"))):
        h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


_CODE_IDS = None


def loaded_code_ids():
    """Machine-code identity of the 512-thread search-kernel symbols of the library this process loaded
    (tools/kernel_code_id.py: sha256 of a symbol's disassembled instructions); {} when the LLVM tools are missing."""
    global _CODE_IDS
    if _CODE_IDS is None:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import kernel_code_id
            from seismic_amd import _native
            _CODE_IDS = kernel_code_id.code_ids(_native.LIB_PATH, r"seismic_search_kernel<unsigned (short|int), 512, ")
        except Exception as e:   # noqa: BLE001  (bookkeeping only: the figure is then reported as unknown)
            print("bench: kernel code ids unavailable: %r" % (e,), file=sys.stderr)
            _CODE_IDS = {}
    return _CODE_IDS


def recorded_traffic(key):
    """roofline.traffic: HBM bytes per launch from SEPARATE rocprofv3 --pmc passes of this command (counters
    cannot be collected from inside this process), recorded in profiles/pmc_traffic.json under the workload
    AND the kernel they were measured on - the kernel source's id, or the machine code of the symbol the passes ran
    (an edit to another instantiation of the template leaves that code as it was); anything else (another workload,
    a kernel edited since) is null."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        ent = pm.get("workloads", {}).get(key)
        if ent and ent.get("kernel_source_id") == kernel_source_id():
            return float(ent["traffic_bytes"]), None
        if ent and ent.get("symbol_code_id"):
            have = loaded_code_ids().get(ent["symbol"].replace("seismic_search_kernel", ""))
            if have == ent["symbol_code_id"]:
                return float(ent["traffic_bytes"]), "recorded at kernel source %s on %s, whose machine code (id %s) is the one in this library (kernel source %s)" % (
                    ent.get("kernel_source_id"), ent["symbol"], have, kernel_source_id())
            return None, "recorded for %s with machine code %s (kernel source %s); this library has %s" % (
                ent["symbol"], ent["symbol_code_id"], ent.get("kernel_source_id"), have)
        if ent:
            return None, "recorded for kernel source %s, this is %s" % (ent.get("kernel_source_id", "(unrecorded)"), kernel_source_id())
    except (OSError, ValueError, KeyError):
        pass
    return None, None


def run_calls(calls, n_threads):
    """Issues the calls (zero-argument callables) from n_threads request threads: thread t takes calls t, t + T, ...
    in order, each call returns before the thread issues its next one. Returns the wall time."""
    if n_threads <= 1 or len(calls) <= 1:
        t0 = time.perf_counter()
        for c in calls:
            c()
        return time.perf_counter() - t0
    errs = []

    def worker(t):
        try:
            for c in calls[t::n_threads]:
                c()
        except BaseException as e:   # surfaces in the main thread
            errs.append(e)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    if errs:
        raise errs[0]
    return dt


DUMP_LIMIT_BYTES = 60_000_000   # (the four .npy files, headers included, stay under 64 MB)


def dump_outputs(dirname, scores, ids, counts, suffix=""):
    """--dump-outputs: one step's result rows as a caller receives them (scores f32 [nq, k], ids and counts as f64, exact
    below 2^53) plus rows.npy, the query rows written: all of them, or a fixed sample (seed 0) that fits DUMP_LIMIT_BYTES."""
    nq = len(counts)
    row_bytes = scores.shape[1] * (4 + 8) + 8 + 8
    rows = np.arange(nq)
    if nq * row_bytes > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(nq, DUMP_LIMIT_BYTES // row_bytes, replace=False))
    os.makedirs(dirname, exist_ok=True)
    for name, a in (("scores", scores[rows].astype(np.float32)), ("ids", ids[rows].astype(np.float64)),
                    ("counts", counts[rows].astype(np.float64)), ("rows", rows.astype(np.float64))):
        np.save(os.path.join(dirname, name + suffix + ".npy"), a)


def main():
    args = parse_args()
    import torch
    import torch.distributed as dist

    from seismic_amd import _native
    from seismic_amd._abi import BuildConfig
    from seismic_amd.sharding import shard_bounds

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    if local_world > 1 and "SGPU_HOST_THREADS" not in os.environ:
        # the ranks of a node share its host cores (and the container's CPU quota): each takes its share for the
        # host-parallel phases (index build, packing at upload, exact search) instead of a full team per rank
        quota_ = cpu_quota()
        cores_ = os.cpu_count() or 1
        team_ = cores_ if quota_ is None else max(1, min(cores_, int(quota_)))
        os.environ["SGPU_HOST_THREADS"] = str(max(1, team_ // local_world))
    if world != args.gpus and world == 1 and args.gpus > 1:
        raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node %d bench.py --gpus %d ..."
                         % (args.gpus, args.gpus))
    if not torch.cuda.is_available() or _native.device_count() < 1:
        raise SystemExit("no GPU visible: the search path has no CPU fallback")
    # SGPU_BENCH_BACKEND=gloo + SGPU_BENCH_ONE_DEVICE=1 lets the N>1 control flow be exercised on a
    # 1-GPU box (all ranks share device 0); the real multi-GPU run uses nccl (RCCL), one GPU per rank.
    backend = os.environ.get("SGPU_BENCH_BACKEND", "nccl")
    if os.environ.get("SGPU_BENCH_ONE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    scaling = args.scaling if args.scaling != "auto" else ("strong" if world > 1 else "weak")

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    n_batches = args.batches or min(args.steps + args.warmup, 64)
    n_batches = max(1, n_batches)

    # ---------------- data + index: rank 0 prepares, the others load its files ----------------
    cfg = BuildConfig.defaults(n_postings=args.n_postings, centroid_fraction=args.centroid_fraction,
                               summary_energy=args.summary_energy, max_fraction=args.max_fraction,
                               min_cluster_size=args.min_cluster_size, doc_cut=15,
                               use_device=0 if args.build_on_host else (local_rank + 1))
    coll = 1 if args.collection == "clustered" else 0
    src_tag = ("%d_%d%s" % (args.docs, args.dim, "_clu" if coll else "")) if not args.documents else \
        ("file_%s_%d" % (os.path.basename(args.documents), os.path.getsize(args.documents)))
    tag = "sgpu2_%s_cw%d_np%d_cf%g_se%g_mf%g_mc%d" % (
        src_tag, args.comp_width, args.n_postings, args.centroid_fraction, args.summary_energy,
        args.max_fraction, args.min_cluster_size)
    cache_dir = args.index_cache or tempfile.gettempdir()
    path = os.path.join(cache_dir, tag + ".idx")
    qpath = os.path.join(cache_dir, tag + "_q%d_b%d_w%d_%s.bin" % (args.queries, n_batches, world, scaling))
    # query sets: strong scaling = the same n_batches global batches on every rank (each takes its
    # shard); weak scaling = n_batches batches per rank
    n_sets = n_batches * (world if scaling == "weak" else 1)
    t_gen = t_build = 0.0

    def prepare(write_files):
        """Documents -> index (a cached file when there is one) -> query sets. Deterministic: every rank
        that runs it holds the same data."""
        index = None
        t_gen = t_build = 0.0
        if os.path.exists(path):
            try:
                index = _native.NativeIndex.load(path)
            except _native.SeismicHipError:   # a stale / truncated file from an interrupted run
                index = None
        need_docs = index is None or not args.queries_file
        docs = None
        if need_docs:
            t0 = time.time()
            docs = _native.read_inner_format(args.documents) if args.documents else _native.synth(args.docs, args.dim, 42, 0, collection=coll)
            t_gen = time.time() - t0
        wrote = True
        if index is None:
            t0 = time.time()
            dim = args.dim if not args.documents else max(args.dim, int(docs[1].max()) + 1)
            index = _native.NativeIndex.build(args.comp_width, dim, *docs, cfg)
            t_build = time.time() - t0
            if write_files and (world > 1 or args.index_cache):
                tmp = "%s.tmp.%d" % (path, os.getpid())
                try:
                    if os.environ.get("SGPU_BENCH_NO_HANDOFF"):   # (test hook: exercise the path below)
                        raise OSError("hand-off disabled by SGPU_BENCH_NO_HANDOFF")
                    index.save(tmp)
                    os.replace(tmp, path)     # the other ranks only ever see a complete file
                except (_native.SeismicHipError, OSError) as e:   # e.g. no room in the temporary directory
                    log("[bench] cannot hand the index over as a file (%s): every rank builds its own" % e)
                    wrote = False
                    if os.path.exists(tmp):
                        os.remove(tmp)
        if args.queries_file:
            allq = _native.read_inner_format(args.queries_file)
        else:
            allq = _native.synth(args.queries * n_sets, int(index.desc.dim), 43, 1, docs, collection=coll)
        if write_files and world > 1 and wrote:
            tmp = "%s.tmp.%d" % (qpath, os.getpid())
            try:
                _native.write_inner_format(tmp, *allq)
                os.replace(tmp, qpath)
            except OSError:
                wrote = False
        return index, allq, t_gen, t_build, wrote

    # rank 0 prepares and hands the index and the query sets over as files; if they cannot be written
    # the other ranks prepare the same data themselves
    handoff = True
    if rank == 0:
        index, allq, t_gen, t_build, handoff = prepare(True)
        log("[bench] documents ready in %.1fs, index built in %.1fs" % (t_gen, t_build))
    barrier()
    if world > 1:
        flag = [handoff]
        dist.broadcast_object_list(flag, src=0)
        handoff = bool(flag[0])
    if rank != 0:
        if handoff:
            index = _native.NativeIndex.load(path)
            allq = _native.read_inner_format(qpath)
        else:
            index, allq, _, _, _ = prepare(False)
    if args.value_type != "f16":   # convert_dataset_into: same lists / blocks / summaries, the forward index re-encoded
        index = index.convert(1 if args.value_type == "fixedu8" else 2)
    t0 = time.time()
    index.upload(local_rank)
    t_up = time.time() - t0
    d = index.desc
    a_off, a_comp, a_val = allq
    n_all = len(a_off) - 1
    if args.queries_file:   # a real query file is one batch (repeated if more steps are asked for)
        args.queries = n_all
        n_batches = 1

    def batch_csr(i):
        """CSR of this rank's part of batch i."""
        if scaling == "weak":
            lo = (rank * n_batches + i) * args.queries if not args.queries_file else 0
            hi = lo + args.queries
        else:
            s, e = shard_bounds(args.queries, world, rank)
            lo, hi = i * args.queries + s, i * args.queries + e
        o0, o1 = int(a_off[lo]), int(a_off[hi])
        return (a_off[lo:hi + 1] - a_off[lo]).astype(np.uint64), a_comp[o0:o1], a_val[o0:o1]

    host_batches = [batch_csr(i) for i in range(n_batches)]
    batches = [_native.DeviceBatch(index, *hb, args.k) for hb in host_batches]
    my_q = len(host_batches[0][0]) - 1
    total_q_per_step = args.queries * (world if scaling == "weak" else 1)
    srt = bool(args.first_sorted)

    # every batch's result rows (the entry point writes into them; no allocation inside the timed region)
    outs = [(np.zeros((my_q, args.k), np.float32), np.zeros((my_q, args.k), np.uint64), np.zeros(max(my_q, 1), np.uint32))
            for _ in range(n_batches)]
    # (a call returns its rows before its thread issues the next one; the host side of a small call - validation, launch
    # plan, staging, copies: ~0.3 us per query - is hidden by the other threads' kernels)
    n_threads = args.host_threads if args.host_threads > 0 else (2 if my_q >= 2500 else 3)

    def entry_call(i):
        b = i % n_batches
        return lambda: index.batch_search(*host_batches[b], args.k, args.query_cut, args.heap_factor, srt, out=outs[b])

    # ---------------- timed region: K calls of the entry point (host buffers in and out) ----------------
    timed_ids = sorted({(args.warmup + i) % n_batches for i in range(args.steps)})
    last = (args.warmup + args.steps - 1) % n_batches   # the batch of the last timed step
    dump_suffix = "" if world == 1 else "_rank%d" % rank
    elapsed, entry_results = None, {}
    if not args.no_entry:
        run_calls([entry_call(i) for i in range(args.warmup)], n_threads)
        barrier()
        t0 = time.perf_counter()
        run_calls([entry_call(args.warmup + i) for i in range(args.steps)], n_threads)
        barrier()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        entry_results = {bi: tuple(a.copy() for a in outs[bi]) for bi in timed_ids[:1]}
        if args.dump_outputs:   # (before any later leg writes into the same rows)
            dump_outputs(args.dump_outputs, outs[last][0], outs[last][1], outs[last][2][:my_q], dump_suffix)
    # N > 1, BASELINE configs[3] read literally: ONE batch at a time - a barrier before and after every step, each rank
    # issues its shard as one call from one thread, so no call of a later batch hides a rank's host side or fills its
    # launch tail. Reported NEXT to `value` (whose K calls are issued back to back from the request threads).
    one_at_a_time = None
    if args.full and world > 1 and scaling == "strong" and not args.no_entry:
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            entry_call(args.warmup + i)()
            barrier()
        dt1 = time.perf_counter() - t0
        t = torch.tensor([dt1], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        one_at_a_time = float(t.item())

    # ---------------- kernel leg (roofline): the same batches resident in HBM, HIP events around each launch ----------------
    if args.full or args.no_entry:
        def step(i):
            batches[i % n_batches].run(args.k, args.query_cut, args.heap_factor, srt, sync=False)

        for i in range(args.warmup):
            step(i)
        batches[0].sync()
        barrier()
        tk0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        sync_stats = batches[0].sync()   # waits for the K launches; mean kernel duration from HIP events
        barrier()
        k_elapsed = time.perf_counter() - tk0
        if world > 1:
            t = torch.tensor([k_elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            k_elapsed = float(t.item())
        kernel_ms = float(sync_stats.kernel_ms)
        if elapsed is None:   # --no-entry: the kernel leg is the timed region
            elapsed = k_elapsed
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, *batches[last].fetch(args.k), dump_suffix)

    ms_per_step = elapsed * 1e3 / args.steps
    qps = total_q_per_step * args.steps / elapsed
    key = workload_key(args, world, scaling)
    out = {
        "metric": METRIC,
        "value": qps,
        "unit": "queries/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "amortized_us_per_query": ms_per_step * 1e3 / total_q_per_step,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic" if not args.documents else "file",
        "config": {
            "workload": ("%s: %d docs, %d vocab, ~%d nnz/doc, best_configs params, "
                         "k=%d, %d-query batch per step%s, %d distinct batches, %s"
                         % (("MSMARCO-passage SPLADE-v3 shape (synthetic%s)" % (", clustered collection" if coll else "")) if not args.documents
                            else "documents %s" % os.path.basename(args.documents),
                            int(d.n_docs), int(d.dim), int(d.nnz) // max(int(d.n_docs), 1), args.k, args.queries,
                            (" sharded over %d GPUs" % world) if (world > 1 and scaling == "strong") else
                            (" per GPU" if world > 1 else ""), n_batches,
                            ("%d ranks on one device" % world) if os.environ.get("SGPU_BENCH_ONE_DEVICE") else "%dxMI355X" % world)),
            "workload_key": key,
            "index": {"n_postings": args.n_postings, "centroid_fraction": args.centroid_fraction,
                      "summary_energy": args.summary_energy, "max_fraction": args.max_fraction,
                      "min_cluster_size": args.min_cluster_size, "doc_cut": 15,
                      "hbm_bytes": index.device_bytes(), "n_blocks": int(d.n_blocks),
                      "n_postings_kept": int(d.n_postings), "summary_entries": int(d.n_entries)},
            "query": {"k": args.k, "query_cut": args.query_cut, "heap_factor": args.heap_factor,
                      "first_sorted": srt},
            "storage": "%s, u8-quantised block summaries" % (
                "fixed-u8 document values, compressed component stream (DotVByte forward index, 2.5 B per element)" if args.value_type == "dotvbyte"
                else "%s document values, u%d components" % (args.value_type, 8 * args.comp_width)),
            "parallelism": "index replicated, %s, no collective" % (
                ("each batch of %d cut into %d contiguous shards" % (args.queries, world)) if scaling == "strong" and world > 1
                else ("%d batch(es) of %d per step" % (world, args.queries))),
            "timed_region": ("K calls of sgpu_batch_search (host buffers in and out) from %d request thread(s)" % n_threads)
            if not args.no_entry else "--no-entry: K device-resident launches (profiling run)",
        },
        "entry_point": {"name": "sgpu_batch_search", "host_threads": n_threads, "queries_per_call": my_q},
        "library": _native.build_info() + (" (matches this tree)" if _native.source_fingerprint() in _native.build_info() else " (NOT the build of this tree: %s)" % _native.source_fingerprint()),
        "timing_s": {"generate": t_gen, "build": t_build, "upload": t_up},
    }
    if world > 1:
        out["value_is"] = ("pipelined: the K sharded batches are issued back to back from %d request thread(s) per rank, so "
                           "calls of consecutive batches overlap on a GPU" % n_threads)
        out["host_threads_per_rank_for_host_phases"] = os.environ.get("SGPU_HOST_THREADS")

    def finish():
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()

    if not args.full:
        finish()
        return

    # ---------------- accounting (outside the timed region) ----------------
    # every timed batch gets one extra pass with the visited set materialised (sgpu_batch_run_counted):
    # identical results, and work counters that exclude re-encountered documents exactly as the
    # reference does -> algorithmic bytes of each launch
    # bytes per document element as stored: f16 2 + 2, fixed-u8 2 + 1, DotVByte 1.5 (12-byte slices of eight components) + 1
    val_bytes = 2 if args.value_type == "f16" else 1
    doc_comp_bytes = None
    if args.value_type == "dotvbyte":   # 1.5 bytes per component in a packed slice, 2 for the documents that keep the raw form
        raw_docs, raw_elems = index.stream_stats()
        raw_share = raw_elems / float(max(int(d.nnz), 1))
        doc_comp_bytes = 1.5 * (1.0 - raw_share) + 2.0 * raw_share
    algo, counted_identical, results = [], True, {}
    entry_identical = True
    agg = np.zeros(8, np.float64)
    for bi in timed_ids:
        b = batches[bi]
        gsc, gid, gn = b.fetch(args.k)
        if bi in entry_results:   # the entry point's rows are the device-resident launch's rows
            esc, eid, en = entry_results[bi]
            entry_identical &= bool(np.array_equal(en[:my_q], gn) and np.array_equal(eid, gid)
                                    and np.array_equal(esc.view(np.uint32), gsc.view(np.uint32)))
        if args.no_accounting:
            results[bi] = (gsc, gid, gn)
            algo.append(0)
            continue
        b.run_counted(args.k, args.query_cut, args.heap_factor, srt)
        csc, cid, cn = b.fetch(args.k)
        counted_identical &= bool(np.array_equal(cn, gn) and np.array_equal(cid, gid)
                                  and np.array_equal(csc.view(np.uint32), gsc.view(np.uint32)))
        ab, counters = b.algorithmic_bytes(args.k, args.comp_width, val_bytes, doc_comp_bytes)
        algo.append(ab)
        agg += counters[:, :8].sum(axis=0)
        results[bi] = (gsc, gid, gn)
    nq_counted = max(1, my_q * len(timed_ids))
    algo_bytes = float(np.mean(algo))
    achieved = algo_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
    traffic_bytes, traffic_note = args.traffic_bytes, None
    if traffic_bytes is None and world == 1:
        traffic_bytes, traffic_note = recorded_traffic(key)
    first = timed_ids[0]
    gsc, gid, gn = results[first]
    out["config"]["launch"] = {"grid": int(sync_stats.grid), "block": int(sync_stats.block),
                               "lds_bytes": int(sync_stats.lds_bytes), "queries_per_launch": my_q}
    out["entry_point"]["rows_identical_to_device_resident_launch"] = entry_identical
    out["device_resident"] = {"value": total_q_per_step * args.steps / k_elapsed, "unit": "queries/s",
                              "ms_per_step": k_elapsed * 1e3 / args.steps,
                              "note": "the same batches already in HBM, results left in HBM: one kernel launch per step (the r01/r02 `value`)"}
    out["roofline"] = {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_GBPS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBPS,
        "traffic": traffic_bytes,
        "traffic_note": traffic_note,
        "kernel": "seismic_search_kernel",
        "kernel_source_id": kernel_source_id(),
        "measured_on": "device-resident launches of the timed batches (HIP events on the library's stream)",
        "kernel_ms": kernel_ms,
        "algorithmic_bytes_per_launch": algo_bytes,
        "bytes_per_query": algo_bytes / max(my_q, 1),
        "docs_scored_per_query": agg[5] / nq_counted,
        "docs_scored_speculatively_per_query": agg[7] / nq_counted,
        "summary_entries_per_query": agg[2] / nq_counted,
        "counted_pass_identical": counted_identical,
        "launches_accounted": len(timed_ids),
    }
    if world > 1:
        # every rank's kernel leg (its shard resident in HBM, HIP events): the first 8-GPU run shows at once whether a GPU lags
        t = torch.zeros(world, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        t[rank] = kernel_ms
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        out["kernel_ms_per_rank"] = [round(float(x), 4) for x in t.tolist()]
    if one_at_a_time is not None:
        out["value_one_batch_at_a_time"] = args.queries * args.steps / one_at_a_time
        out["one_batch_at_a_time"] = {
            "value": args.queries * args.steps / one_at_a_time, "unit": "queries/s", "ms_per_step": one_at_a_time * 1e3 / args.steps,
            "note": "a barrier around every step, each rank's shard = one sgpu_batch_search call from one thread "
                    "(BASELINE configs[3] read literally; includes one barrier per step)"}

    # ---- N>1, strong scaling: the sharded batch must be the 1-GPU answer, in input order ----
    if world > 1 and scaling == "strong":
        from seismic_amd.sharding import gather_rows
        full = gather_rows(gsc, gid, gn, args.queries)
        if rank == 0:
            lo, hi = first * args.queries, (first + 1) * args.queries
            o0, o1 = int(a_off[lo]), int(a_off[hi])
            ref = index.batch_search((a_off[lo:hi + 1] - a_off[lo]).astype(np.uint64), a_comp[o0:o1], a_val[o0:o1],
                                     args.k, args.query_cut, args.heap_factor, srt)
            out["sharded_identical_to_single_gpu"] = bool(
                np.array_equal(ref[2], full[2]) and np.array_equal(ref[1], full[1])
                and np.array_equal(ref[0].view(np.uint32), full[0].view(np.uint32)))

    # ---- N>1: the same GPUs as N independent replicas (weak scaling), reported NEXT to `value`: every
    # rank searches a whole batch of args.queries per step (rank r starts at batch r), same barriers,
    # same max-over-ranks clock. Strong scaling pays the launch tail of 1/N-size launches; this leg does not.
    if world > 1 and scaling == "strong" and not args.no_weak_leg:
        def whole(i):
            lo, hi = i * args.queries, (i + 1) * args.queries
            o0, o1 = int(a_off[lo]), int(a_off[hi])
            return (a_off[lo:hi + 1] - a_off[lo]).astype(np.uint64), a_comp[o0:o1], a_val[o0:o1]
        wb = [_native.DeviceBatch(index, *whole((i + rank) % n_batches), args.k) for i in range(n_batches)]
        for i in range(args.warmup):
            wb[i % n_batches].run(args.k, args.query_cut, args.heap_factor, srt, sync=False)
        wb[0].sync()
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            wb[(args.warmup + i) % n_batches].run(args.k, args.query_cut, args.heap_factor, srt, sync=False)
        wstats = wb[0].sync()
        barrier()
        welapsed = time.perf_counter() - t0
        t = torch.tensor([welapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        welapsed = float(t.item())
        out["replicas_weak_scaling"] = {
            "value": world * args.queries * args.steps / welapsed, "unit": "queries/s",
            "ms_per_step": welapsed * 1e3 / args.steps, "queries_per_gpu_per_step": args.queries,
            "kernel_ms_rank0": float(wstats.kernel_ms),
            "note": "N independent replicas, one whole batch per GPU and step; `value` above is ONE batch sharded over the GPUs",
        }
        del wb

    if rank == 0 and args.results_tsv:
        _native.write_results_tsv(args.results_tsv, gsc, gid, gn)
    if rank == 0 and args.groundtruth:
        from seismic_amd.index import accuracy, read_results_tsv
        res = {q: [int(x) for x in gid[q, :gn[q]]] for q in range(len(gn))}
        out["accuracy_vs_groundtruth"] = accuracy(res, read_results_tsv(args.groundtruth))

    ns = min(args.sample, my_q)
    s_off, s_comp, s_val = host_batches[first]
    s_off = s_off[:ns + 1].copy()
    s_comp, s_val = s_comp[:int(s_off[ns])], s_val[:int(s_off[ns])]

    # the single-GPU legs (end to end, batch-1 latency, recall, cpu_baseline) belong to the N=1 line
    if world > 1 and not args.all_legs:
        args.no_e2e = args.no_latency = args.no_recall = True
        out["single_gpu_legs"] = "skipped at N>1 (end_to_end, latency, recall, cpu_baseline: see the N=1 line; --all-legs runs them)"
    if rank == 0 and not args.no_e2e:
        # the entry point from other numbers of request threads, on the timed batches (secondary: `value` above
        # is the timed region itself, args.host_threads threads)
        calls = [entry_call(args.warmup + i) for i in range(args.steps)]
        e2e = {"entry_point": "sgpu_batch_search (host buffers in and out)", "queries_per_call": my_q, "calls": len(calls)}
        for nt in (1, 2, 3):
            run_calls(calls[:nt], nt)
            dt = run_calls(calls, nt)
            e2e["qps_%d_host_thread%s" % (nt, "" if nt == 1 else "s")] = my_q * len(calls) / dt
            if nt == 1:
                e2e["ms_per_call"] = dt * 1e3 / len(calls)
        out["end_to_end"] = e2e

    if rank == 0 and not args.no_latency:
        # mean latency of batch-1 searches: the reference's AQT loop (one query at a time,
        # src/bin/perf_inverted_index.rs:184-216) natively - sgpu_search_sequential = one sgpu_search per query,
        # host buffers in and out, timed around the loop - over the whole sample, three passes
        runs, phases, each = [], None, []
        index.search_sequential(s_off[:11], s_comp, s_val, args.k, args.query_cut, args.heap_factor, srt)
        for rep in range(3):
            lsc, lid, ln, mean_us, ph, per_q = index.search_sequential(s_off, s_comp, s_val, args.k, args.query_cut, args.heap_factor, srt,
                                                                       per_query=True)
            runs.append(mean_us)
            each.append(per_q)
            phases = ph if phases is None else phases + ph
        each = np.concatenate(each)
        out["mean_latency_us_single_query"] = float(np.mean(runs))
        out["latency_percentiles_us_single_query"] = {
            "p50": float(np.percentile(each, 50)), "p95": float(np.percentile(each, 95)), "p99": float(np.percentile(each, 99)),
            "max": float(each.max()), "min": float(each.min()), "mean": float(each.mean()), "calls": int(len(each)),
            "note": "wall time of every sgpu_search call of the three passes (sgpu_search_sequential_timed)"}
        out["latency"] = {
            "entry_point": "sgpu_search, one call per query, sequential (sgpu_search_sequential)",
            "queries": ns, "passes_mean_us": runs,
            "host_phases_us": {n_: float(v_) / 3 for n_, v_ in zip(
                ["validate_plan", "staging", "enqueue_h2d", "configure_launch", "enqueue_d2h", "wait_kernel_runs_here", "copy_out"], phases[:7])},
            "rows_identical_to_batch": bool(np.array_equal(ln, gn[:ns]) and np.array_equal(lid, gid[:ns])
                                            and np.array_equal(lsc.view(np.uint32), gsc[:ns].view(np.uint32))),
            "reference_published_us": 185.0,   # README.md:110-115 (Core Ultra 7 265K, real MS MARCO; other data, other host)
        }
        # the same calls one by one through the ctypes binding: three passes, the median reported and all three kept -
        # a pass that meets one scheduler stall of the container (the GPU boxes run under a 16-CPU cgroup quota; a
        # throttled period parks the process for tens of milliseconds) reads 200 us per call higher than its
        # neighbours (profiles/r03_binding_probe.txt: 153 / 352 / 148 us for identical passes)
        nlat = min(200, ns)
        py_passes = []
        for rep in range(3):
            t0 = time.perf_counter()
            for i in range(nlat):
                index.search(s_comp[int(s_off[i]):int(s_off[i + 1])], s_val[int(s_off[i]):int(s_off[i + 1])], args.k,
                             args.query_cut, args.heap_factor, srt)
            py_passes.append((time.perf_counter() - t0) * 1e6 / max(nlat, 1))
        out["latency"]["through_python_binding_us"] = float(np.median(py_passes))   # (median of the three passes)
        out["latency"]["through_python_binding_passes_us"] = py_passes
        singles = [_native.DeviceBatch(index, np.array([0, int(s_off[i + 1] - s_off[i])], np.uint64),
                                       s_comp[int(s_off[i]):int(s_off[i + 1])], s_val[int(s_off[i]):int(s_off[i + 1])], args.k)
                   for i in range(min(50, ns))]
        kms = 0.0
        for sb in singles:
            kms += sb.run(args.k, args.query_cut, args.heap_factor, srt, sync=True).kernel_ms
        out["mean_kernel_us_single_query"] = kms * 1e3 / max(len(singles), 1)
        del singles

    exact_ids = None
    if rank == 0 and not args.no_recall:
        t0 = time.time()
        # exact top-k (host, all documents) of the sample AND of the held-out queries [ns, ns + nh) of the same batch:
        # parameters of the operating points are selected on the sample, their recall is reported on the held-out queries
        nh = max(0, min(args.heldout, my_q - ns)) if (world == 1 and args.target_recall.strip()) else 0
        x_off, x_comp, x_val = host_batches[first]
        x_off = x_off[:ns + nh + 1].copy()
        es, ei, en = index.exact_search(x_off, x_comp[:int(x_off[ns + nh])], x_val[:int(x_off[ns + nh])], args.k)
        exact_ids = [set(ei[i, :en[i]].tolist()) for i in range(ns + nh)]

        def recall_of(ids, n, lo=0, hi=None):
            hi = ns if hi is None else hi
            return sum(len(set(ids[i, :n[i]].tolist()) & exact_ids[i]) for i in range(lo, hi)) / float(max(hi - lo, 1) * args.k)
        out["recall_at_k"] = recall_of(gid, gn)
        out["recall_sample_queries"] = ns
        if nh:
            out["recall_heldout"] = recall_of(gid, gn, ns, ns + nh)
            out["recall_heldout_queries"] = nh
        out["timing_s"]["exact_ground_truth"] = time.time() - t0

    if rank == 0 and world == 1 and exact_ids is not None and args.target_recall.strip():
        try:
            # ---- operating points at fixed recall (the metric is "at fixed recall@10") the way the reference makes them:
            # a recall target is reached through INDEX parameters (n_postings, max_fraction) with a small query_cut, one
            # index per target (experiments/best_configs/msmarco-v1/splade-v3/mem_budget_2.0/recall_90 ... recall_99.toml
            # differ in n-postings 2000/3000/4000, max-fraction 2/3/4/6, query-cut 4/6, heap-factor 0.9/1.0). The index
            # parameters per target come from profiles/operating_points.json - the cheapest of a sweep over index AND query
            # parameters on this collection (tools/operating_sweep.py, a GPU run of minutes; committed with its raw points).
            # Here every target's index is built, its query parameters are re-selected on THIS run's sample among the
            # recorded point and its neighbours (cheapest whole-batch kernel time that reaches the target), and the point
            # is measured like the headline: entry point, device-resident launches, counted pass -> roofline, single-query
            # latency, results identical to the CPU oracle, and the CPU oracle timed at the same parameters.
            import orc
            t0 = time.time()
            targets = [float(x) for x in args.target_recall.split(",") if x.strip()]
            try:
                recorded = json.load(open(os.path.join(ROOT, "profiles", "operating_points.json")))
            except (OSError, ValueError):
                recorded = {"targets": []}
            rec_by_t = {round(float(t_["target_recall"]), 4): t_ for t_ in recorded.get("targets", [])}
            head_idx = {"n_postings": args.n_postings, "max_fraction": args.max_fraction,
                        "centroid_fraction": args.centroid_fraction, "summary_energy": args.summary_energy}
            quota = cpu_quota()
            ncores = os.cpu_count() or 1
            cpu_threads = ncores if quota is None else max(2, min(ncores, int(quota)))
            points = []
            measured = {}   # (index, query parameters) -> (whole-batch kernel ms, sample recall): targets share their measurements
            built = {}   # index parameters -> (index, resident batches); at most one extra index is alive at a time

            def index_for(ip):
                key_ = json.dumps(ip, sort_keys=True)
                if ip == head_idx:
                    return index, batches, 0.0, 0.0
                if key_ in built:
                    return built[key_]
                for v_ in list(built.values()):   # free the previous target's index before the next one is built
                    for b_ in v_[1]:
                        b_.close()
                    v_[0].close()
                built.clear()
                t1 = time.time()
                docs_ = _native.read_inner_format(args.documents) if args.documents else _native.synth(args.docs, args.dim, 42, 0, collection=coll)
                cfg_ = BuildConfig.defaults(n_postings=int(ip["n_postings"]), centroid_fraction=float(ip["centroid_fraction"]),
                                            summary_energy=float(ip["summary_energy"]), max_fraction=float(ip["max_fraction"]),
                                            min_cluster_size=args.min_cluster_size, doc_cut=15,
                                            use_device=0 if args.build_on_host else (local_rank + 1))
                ix_ = _native.NativeIndex.build(args.comp_width, int(d.dim), *docs_, cfg_)
                del docs_
                tb_ = time.time() - t1
                if args.value_type != "f16":
                    ix_ = ix_.convert(1 if args.value_type == "fixedu8" else 2)
                t1 = time.time()
                ix_.upload(local_rank)
                tu_ = time.time() - t1
                nb_ = min(5, n_batches)
                bs_ = [_native.DeviceBatch(ix_, *host_batches[(first + j) % n_batches], args.k) for j in range(nb_)]
                built[key_] = (ix_, bs_, tb_, tu_)
                return built[key_]

            def measure(ix_, bs_, cut, hf, fs):
                """One (query_cut, heap_factor, first_sorted) on resident batch 0 of bs_ (it holds the sample): kernel ms of the
                whole-batch launch (best of two), recall@k of the sample rows (selection) and of the held-out rows (report)."""
                bs_[0].run(args.k, cut, hf, fs)
                ms_ = min(bs_[0].run(args.k, cut, hf, fs).kernel_ms for _ in range(2))
                _, pid_, pn_ = bs_[0].fetch(args.k)
                return float(ms_), recall_of(pid_, pn_), (recall_of(pid_, pn_, ns, ns + nh) if nh else None)

            # the recorded points belong to the collection they were swept on
            rec_applies = (not args.documents and coll == 0 and recorded.get("docs") == args.docs and recorded.get("dim") == args.dim
                           and args.comp_width == 2)
            for tgt in targets:
                rec = rec_by_t.get(round(tgt, 4)) if rec_applies else None
                if rec is not None and not rec.get("reached", False):
                    rec = None
                cands = set()
                if rec is None:
                    # no recorded point for this target / collection: the query-parameter grid on the headline index
                    ip = dict(head_idx)
                    for cut_ in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16):
                        for hf_ in (0.7, 0.8, 0.9, 1.0):
                            for fs_ in (False, True):
                                cands.add((cut_, hf_, fs_))
                else:
                    ip = {k_: rec["best"]["index"][k_] for k_ in ("n_postings", "max_fraction", "centroid_fraction", "summary_energy")}
                ix_, bs_, tb_, tu_ = index_for(ip)
                same_index = ip == head_idx
                if same_index:   # batch `first` holds the sample
                    bs_ = [batches[(first + j) % n_batches] for j in range(min(5, n_batches))]
                # candidates: the recorded point and runners-up on the same index, plus their neighbours in query_cut / heap_factor
                for r_ in ([rec["best"]] + list(rec.get("runners_up", []))) if rec is not None else []:
                    if {k_: r_["index"][k_] for k_ in ip} != ip:
                        continue
                    for dc in (-1, 0, 1, 2):
                        for hf_ in sorted({float(r_["heap_factor"]), 1.0, 0.9}):
                            if int(r_["query_cut"]) + dc >= 1:
                                cands.add((int(r_["query_cut"]) + dc, hf_, bool(r_["first_sorted"])))
                tried = []
                for cut, hf, fs in sorted(cands):
                    mkey = (json.dumps(ip, sort_keys=True), cut, hf, fs)
                    if mkey not in measured:
                        measured[mkey] = measure(ix_, bs_, cut, hf, fs)
                    ms_, rc_, rh_ = measured[mkey]
                    tried.append({"query_cut": cut, "heap_factor": hf, "first_sorted": fs, "recall": rc_, "recall_heldout": rh_,
                                  "batch_kernel_ms": ms_})
                # SELECTION looks at the sample only (queries 0 .. ns-1): the cheapest candidate whose sample recall clears
                # the target by a margin of two standard errors of a recall measured on ns x k slots (the sample estimate of
                # a point that sits exactly on the target is below it half of the time); without such a candidate, the
                # cheapest one that reaches the target on the sample. The point's recall is then REPORTED on the held-out
                # queries, which played no part in the choice, and it counts as reached only if that figure meets the target.
                margin = 2.0 * (tgt * (1.0 - tgt) / float(max(ns, 1) * args.k)) ** 0.5 if nh else 0.0
                ok = [g for g in tried if g["recall"] >= tgt + margin] or [g for g in tried if g["recall"] >= tgt]
                if not ok:
                    best = max(tried, key=lambda g: g["recall"])
                    points.append({"target_recall": tgt, "reached": False, "index": ip, "best_recall_on_grid": best["recall"],
                                   "best_recall_heldout": best["recall_heldout"],
                                   "at": {k_: best[k_] for k_ in ("query_cut", "heap_factor", "first_sorted")}, "tried": len(tried)})
                    continue
                g = min(ok, key=lambda g: g["batch_kernel_ms"])
                cut, hf, fs = g["query_cut"], g["heap_factor"], g["first_sorted"]
                nb_ = len(bs_)
                sel = [(first + j) % n_batches for j in range(nb_)]
                # the entry-point leg takes host buffers only: up to twelve distinct batches (with five calls the last one,
                # running alone, is a fifth of the measurement)
                sel_e = [(first + j) % n_batches for j in range(min(n_batches, 12))]
                calls = [(lambda b_=b_: ix_.batch_search(*host_batches[b_], args.k, cut, hf, fs, out=outs[b_])) for b_ in sel_e]
                run_calls(calls[:n_threads], n_threads)
                dt_e = run_calls(calls, n_threads)
                bs_[0].sync()   # (resets the library's running mean of kernel durations)
                for b_ in bs_:
                    b_.run(args.k, cut, hf, fs, sync=False)
                st_ = bs_[0].sync()
                bs_[0].run_counted(args.k, cut, hf, fs)
                ab, cst = bs_[0].algorithmic_bytes(args.k, args.comp_width, val_bytes, doc_comp_bytes)
                psc, pid, pn = bs_[0].fetch(args.k)
                dx = ix_.desc
                osc, oid, on_, _, secs_1, _ = orc.batch_search(dx, s_off, s_comp, s_val, args.k, cut, hf, fs, num_threads=1, tuned=True)
                best_n, used_n = 0.0, cpu_threads
                if not args.no_cpu:
                    for rep in range(3):   # all-core: the quota-capped team, best of the second and third pass
                        r_ = orc.batch_search(dx, s_off, s_comp, s_val, args.k, cut, hf, fs, num_threads=cpu_threads, tuned=True)
                        if rep:
                            best_n = max(best_n, ns / r_[4])
                        used_n = int(r_[5])
                # single-query latency on held-out queries (the first 300 behind the sample), with its distribution
                l0_, l1_ = (ns, min(ns + 300, ns + nh)) if nh else (0, min(ns, 300))
                l_off = (x_off[l0_:l1_ + 1] - x_off[l0_]).astype(np.uint64)
                l_comp, l_val = x_comp[int(x_off[l0_]):int(x_off[l1_])], x_val[int(x_off[l0_]):int(x_off[l1_])]
                ix_.search_sequential(l_off[:11], l_comp, l_val, args.k, cut, hf, fs)
                _, _, _, lat_us, _, lat_each = ix_.search_sequential(l_off, l_comp, l_val, args.k, cut, hf, fs, per_query=True)
                pa = argparse.Namespace(**vars(args))
                pa.n_postings, pa.max_fraction = int(ip["n_postings"]), float(ip["max_fraction"])
                pa.centroid_fraction, pa.summary_energy = float(ip["centroid_fraction"]), float(ip["summary_energy"])
                pa.query_cut, pa.heap_factor, pa.first_sorted = cut, hf, int(fs)
                pkey = workload_key(pa, world, scaling)
                ptraffic, pnote = recorded_traffic(pkey)
                kms_ = float(st_.kernel_ms)
                held = g["recall_heldout"]
                pt = {"target_recall": tgt, "reached": bool((held if held is not None else g["recall"]) >= tgt),
                      "index": dict(ip, hbm_bytes=ix_.device_bytes(), build_s=tb_, upload_s=tu_, same_as_headline=same_index),
                      "query_cut": cut, "heap_factor": hf, "first_sorted": fs,
                      "recall_at_k": held if held is not None else g["recall"],
                      "recall_selection_sample": g["recall"], "recall_heldout": held,
                      "recall_queries": {"selection": [0, ns], "heldout": [ns, ns + nh], "selection_margin": margin},
                      "latency_percentiles_us": {"p50": float(np.percentile(lat_each, 50)), "p95": float(np.percentile(lat_each, 95)),
                                                 "p99": float(np.percentile(lat_each, 99)), "max": float(lat_each.max()),
                                                 "queries": [int(l0_), int(l1_)]},
                      "value": my_q * len(calls) / dt_e, "unit": "queries/s", "entry_point_calls": len(calls),
                      "device_resident_qps": my_q / (kms_ * 1e-3) if kms_ > 0 else None,
                      "kernel_ms": kms_, "mean_latency_us_single_query": lat_us,
                      "roofline_frac": ab / (kms_ * 1e-3) / 1e9 / HBM_PEAK_GBPS if kms_ > 0 else None,
                      "algorithmic_bytes_per_launch": ab, "traffic": ptraffic, "traffic_note": pnote, "workload_key": pkey,
                      "docs_scored_per_query": float(cst[:, 5].mean()), "launch": {"grid": int(st_.grid), "lds_bytes": int(st_.lds_bytes)},
                      "candidates_tried": len(tried)}
                pt["identical_to_cpu_oracle_on_sample"] = bool(
                    np.array_equal(on_, pn[:ns]) and np.array_equal(oid, pid[:ns])
                    and np.array_equal(osc.view(np.uint32), psc[:ns].view(np.uint32)))
                pt["cpu_baseline"] = {"single_thread_us_per_query": secs_1 * 1e6 / ns, "value": best_n if best_n > 0 else None,
                                      "unit": "queries/s", "cores": used_n, "kind": "port",
                                      "sample": "the %d sample queries at this point's parameters: one single-thread pass, "
                                                "best of two passes on %d pinned threads" % (ns, used_n)}
                if best_n > 0:
                    pt["gpu_over_cpu_allcore"] = pt["value"] / best_n
                points.append(pt)
            for v_ in list(built.values()):
                for b_ in v_[1]:
                    b_.close()
                v_[0].close()
            built.clear()
            out["operating_points"] = points
            out["operating_points_source"] = {
                "file": "profiles/operating_points.json", "sweep": recorded.get("sweep"),
                "selection": "per target the cheapest whole-batch kernel time among index AND query parameters (tools/operating_sweep.py); "
                             "query parameters re-selected here on this run's %d-query sample among the recorded point and its neighbours; "
                             "recall REPORTED on %d held-out queries of the same batch (a point is `reached` only if the held-out recall "
                             "meets its target)" % (ns, nh)}
            out["timing_s"]["operating_points"] = time.time() - t0
        except Exception as e:   # (the headline line must survive a failure of this leg: it is reported, not raised)
            import traceback
            out["operating_points_error"] = "%s: %s" % (type(e).__name__, e)
            log("[bench] operating points leg failed:\n" + traceback.format_exc())

    if rank == 0 and world == 1 and not args.no_cpu:
        # ---- cpu_baseline: the CPU oracle's tuned path (a port; the Rust reference cannot be built here:
        # AVX2 + F16C scorer, hash-set visited set, whole-document prefetch, pinned threads - bit-identical to the
        # restatement, tests/test_oracle_kat.py), timed on this box's host cores on the same index and a bounded
        # sample of the same queries.
        import orc
        ncores = os.cpu_count() or 1
        q = (s_off, s_comp, s_val)
        kw = dict(tuned=True)
        singles = []
        for _ in range(3):   # single thread: three passes over the sample, the fastest one is reported
            osc, oid, on, ost, secs1, _ = orc.batch_search(d, *q, args.k, args.query_cut, args.heap_factor, srt, num_threads=1, **kw)
            singles.append(secs1)
        secs1 = min(singles)
        identical = bool(np.array_equal(on, gn[:ns]) and np.array_equal(oid, gid[:ns])
                         and np.array_equal(osc.view(np.uint32), gsc[:ns].view(np.uint32)))
        qps1 = ns / secs1
        # many cores: one query per task (the reference's rayon pool), threads pinned. Thread counts up to every
        # hardware thread are tried; each is timed on its second and third pass, the best one is then run for the
        # rest of the budget.
        # A container CPU quota (cgroup cpu.max) bounds what can be sustained: threads beyond it only borrow from the
        # current accounting period and are throttled afterwards (a one-second sample looks 1.6 x faster at twice
        # the quota than anything longer can be: profiles/r03_cpu_thread_sweep.txt), so the sweep stays within it.
        quota = cpu_quota()
        limit = ncores if quota is None else max(2, min(ncores, int(quota)))
        sweep = {}
        t_sweep = time.time()
        for nt in sorted({c for c in (limit, limit // 2, limit // 4, 128, 64, 32, 16) if 2 <= c <= limit}):
            best = 0.0
            for rep in range(3):
                r = orc.batch_search(d, *q, args.k, args.query_cut, args.heap_factor, srt, num_threads=nt, **kw)
                if rep:
                    best = max(best, ns / r[4])
            sweep[int(r[5])] = best
            if time.time() - t_sweep > args.cpu_seconds / 2:
                break
        used = max(sweep, key=sweep.get)
        runs_n, t_n = 0, 0.0
        while t_n < args.cpu_seconds / 2 and runs_n < 512:
            t_n += orc.batch_search(d, *q, args.k, args.query_cut, args.heap_factor, srt, num_threads=used, **kw)[4]
            runs_n += 1
        qpsn = max(runs_n * ns / t_n, sweep[used])
        out["cpu_baseline"] = {
            "value": qpsn, "unit": "queries/s", "cores": int(used), "kind": "port",
            "sample": "the first %d queries of the first timed batch: %d passes on %d pinned OpenMP threads (one query "
                      "per task) after a thread-count sweep; single thread: fastest of 3 passes. The host has %d hardware "
                      "threads; the container may use %s CPUs' worth of time (cgroup quota), which caps the team"
                      % (ns, runs_n, used, ncores, "all" if quota is None else ("%g" % quota)),
            "single_thread_qps": qps1, "single_thread_us_per_query": 1e6 / qps1,
            "single_thread_passes_us_per_query": [x * 1e6 / ns for x in singles],
            "host_cores": ncores, "cpu_quota_cpus": quota, "thread_sweep_qps": {str(k_): v_ for k_, v_ in sorted(sweep.items())},
            "gpu_results_identical_to_cpu": identical,
            "implementation": "oracle/seismic_oracle.cpp search_one<true>: AVX2+F16C scorer, hash-set visited set, range prefetch",
        }
        out["gpu_over_cpu_allcore"] = qps / qpsn if qpsn > 0 else None
    finish()


if __name__ == "__main__":
    main()
