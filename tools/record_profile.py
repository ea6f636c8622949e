#!/usr/bin/env python3
"""Copies what tools/profile_bench.sh / tools/profile_traffic.sh wrote under gpurun_out/ into profiles/ and records the
measured HBM traffic in profiles/pmc_traffic.json under the workload AND the kernel source id it was measured on.
  python tools/record_profile.py bench   gpurun_out/r03_prof2 r03      -> profiles/r03_{kernel_stats.csv,rocprof_summary.json,bench_under_rocprof.json,pmc.md}
  python tools/record_profile.py traffic gpurun_out/r03_traffic_c5 r03_traffic_c5"""
import json, os, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_code_id  # noqa: E402
mode, src, tag = sys.argv[1], os.path.join(ROOT, sys.argv[2]), sys.argv[3]
P = os.path.join(ROOT, "profiles")
s = json.load(open(os.path.join(src, "summary.json")))
first = "trace_bench.json" if os.path.exists(os.path.join(src, "trace_bench.json")) else "pmc_FETCH_SIZE.json"
line = json.loads(open(os.path.join(src, first)).read().strip().splitlines()[-1])
pmc_line = json.loads(open(os.path.join(src, "pmc_FETCH_SIZE.json")).read().strip().splitlines()[-1])


def timed_kernel(table):
    best = None
    for k, c in table.items():
        if not k.startswith("seismic_search_kernel<"):
            continue
        # template arguments: component type, threads, heap registers, lookup, COUNTED, value type, COOP[, STREAM (r06)]
        targs = [x.strip() for x in k[k.index("<") + 1:k.rindex(">")].split(",")]
        if targs[4] == "false" and targs[6] == "false":   # the timed variants: neither the counted pass nor a cooperative launch
            d = next(iter(c.values()))["dispatches"]
            if best is None or d > best[1]:
                best = (k, d)
    return best[0]


K = timed_kernel(s["counters"]["pmc_FETCH_SIZE"])
f, w = s["counters"]["pmc_FETCH_SIZE"][K]["FETCH_SIZE"], s["counters"]["pmc_WRITE_SIZE"][K]["WRITE_SIZE"]
ent = {"traffic_bytes": int(2 * f["mean"] * 1024 + w["mean"] * 1024), "fetch_size_kib": int(f["mean"]), "write_size_kib": int(w["mean"]),
       # the id over ALL the kernel's source files (the tree that ran travels with the library). It is not the id bench.py
       # computes - that one leaves out search_kernel.inc's parts -, so bench never accepts this entry on source alone: its
       # comparison of the symbol's machine code (below) decides
       "dispatches": f["dispatches"], "kernel_source_id": kernel_code_id.kernel_source_id_full(),
       "algorithmic_bytes": line["roofline"]["algorithmic_bytes_per_launch"]}
ent["ratio"] = round(ent["traffic_bytes"] / ent["algorithmic_bytes"], 4) if ent["algorithmic_bytes"] else None
# the symbol the counter passes ran and the identity of its machine code in the library of this tree (the one that ran:
# the .so travels to the GPU box with the snapshot) - bench.py reports the figure for that code only
ent["symbol"] = K
try:
    ent["symbol_code_id"] = kernel_code_id.code_ids(None, r"seismic_search_kernel<").get(K.replace("seismic_search_kernel", ""))
except Exception as e:   # noqa: BLE001
    print("record_profile: no machine-code id (%r)" % (e,), file=sys.stderr)
pm = json.load(open(os.path.join(P, "pmc_traffic.json")))
key = pmc_line["config"]["workload_key"]
if mode == "traffic":
    ent["recorded"] = "%s (profiles/%s.json, tools/profile_traffic.sh)" % (tag.split("_")[0], tag)
    shutil.copy(os.path.join(src, "summary.json"), os.path.join(P, tag + ".json"))
    pm["workloads"][key] = ent
    json.dump(pm, open(os.path.join(P, "pmc_traffic.json"), "w"), indent=1)
    print(key, ent)
    sys.exit(0)
ent["recorded"] = "%s (profiles/%s_rocprof_summary.json, tools/profile_bench.sh)" % (tag, tag)
ent["forward_store"] = "block-major"
pm["workloads"][key] = ent
json.dump(pm, open(os.path.join(P, "pmc_traffic.json"), "w"), indent=1)
shutil.copy(os.path.join(src, "trace", "trace_kernel_stats.csv"), os.path.join(P, tag + "_kernel_stats.csv"))
shutil.copy(os.path.join(src, "summary.json"), os.path.join(P, tag + "_rocprof_summary.json"))
shutil.copy(os.path.join(src, "trace_bench.json"), os.path.join(P, tag + "_bench_under_rocprof.json"))
c = s["counters"]


def get(name):
    for v in c.values():
        if K in v and name in v[K]:
            return v[K][name]["mean"]
    return None


names = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_INSTS_VALU",
         "SQ_INSTS_LDS", "TCC_HIT_sum", "TCC_MISS_sum", "SQ_INSTS_VMEM_RD", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT", "SQ_BUSY_CYCLES", "GRBM_GUI_ACTIVE"]
v = {n: get(n) for n in names}
ks = [k for k in s["kernel_stats"] if k["kernel"] == K][0]
cnt = [k for k in s["kernel_stats"] if k["kernel"].startswith("seismic_search_kernel") and ", true, " in k["kernel"]]
kms = line["roofline"]["kernel_ms"]
cyc = kms * 1e-3 * 2.4e9
md = """# %s — rocprofv3 passes of the headline workload (tools/profile_bench.sh, `bench.py --no-entry`: every dispatch of the
search kernel is one whole 10 000-query batch; kernel source id %s)

Kernel trace (`%s_kernel_stats.csv`): timed variant `%s`: %d calls, average %.1f us (min %.1f, max %.1f = the first
warm-up launch); `bench.py` under the profiler measured kernel_ms %.3f by HIP events (`%s_bench_under_rocprof.json`).
%s

| counter (mean per timed dispatch, %d dispatches per pass) | value |
|---|---|
%s

Derived: HBM traffic = 2 x FETCH_SIZE + WRITE_SIZE (gfx950 correction, MI355X_MICROARCH.md; calibrated in r02 on a
known-bytes kernel of the same access pattern) = %.2f GB per launch = **%.3f x the algorithmic bytes** (%.2f GB);
L2 hit rate %.1f %%; waves parked (SQ_WAIT_ANY / SQ_WAVE_CYCLES) %.1f %%.

The three walls of the scoring loop, per launch of %.2f ms (%.2e shader cycles at 2.4 GHz; 256 CUs x 4 SIMDs):
* **VALU issue: %.3g wave-instructions x 4 cycles = %.0f %% of the SIMD issue slots** (SQ_INSTS_VALU; the ~15 %% "of wave
  cycles" figure quoted in r02 divides by resident-wave cycles, not by issue slots);
* **LDS: SQ_LDS_IDX_ACTIVE / 256 CUs = %.0f %% of the launch's cycles**, of which bank conflicts %.0f %%; %.3g DS wave-instructions;
* **memory: %.0f %% of the 8 TB/s peak by algorithmic bytes, ~%.0f %% of the 6.3 TB/s a streaming copy reaches** once the traffic is counted.
None is saturated alone; each is within reach of the others, which is why trading one for another loses
(`r03_lds_sensitivity.md`: one DS read less for four VALU operations more is 11 %% slower).
""" % (tag, ent["kernel_source_id"], tag, K, ks["calls"], ks["avg_us"], ks["min_us"], ks["max_us"], kms, tag,
       ("The accounting variant (visited bitmap) is its own symbol: %d calls, average %.1f us." % (cnt[0]["calls"], cnt[0]["avg_us"])) if cnt else "",
       f["dispatches"],
       "\n".join("| %s | %s |" % (n, ("%.4g" % x) if x is not None else "-") for n, x in list(v.items()) + [("FETCH_SIZE (KiB)", f["mean"]), ("WRITE_SIZE (KiB)", w["mean"])]),
       ent["traffic_bytes"] / 1e9, ent["ratio"], ent["algorithmic_bytes"] / 1e9,
       100 * v["TCC_HIT_sum"] / (v["TCC_HIT_sum"] + v["TCC_MISS_sum"]), 100 * v["SQ_WAIT_ANY"] / v["SQ_WAVE_CYCLES"],
       kms, cyc, v["SQ_INSTS_VALU"], 100 * v["SQ_INSTS_VALU"] * 4 / (cyc * 1024), 100 * v["SQ_LDS_IDX_ACTIVE"] / 256 / cyc,
       100 * v["SQ_LDS_BANK_CONFLICT"] / v["SQ_LDS_IDX_ACTIVE"], v["SQ_INSTS_LDS"],
       100 * line["roofline"]["frac"], 100 * ent["traffic_bytes"] / (kms * 1e-3) / 6.3e12)
open(os.path.join(P, tag + "_pmc.md"), "w").write(md)
print(key, ent)
print(md)
