"""Device timeline of sgpu_batch_search calls from a rocprofv3 --kernel-trace csv.
  python tools/e2e_timeline.py trace.csv [last]            start / end of the last kernels relative to the first kernel of their
                                                           call (calls are separated by gaps with no kernel resident)
  python tools/e2e_timeline.py trace.csv --calls K [--chunks C]
      the last K calls (the timed steps of `bench.py --steps K` run under the profiler), read per call and per lane: a call
      is C consecutive search launches of one host thread (Thread_Id; default 2), a lane is a stream (Stream_Id). For every
      search launch: start, end and duration (us from the call's first kernel), the plan kernels ahead of it on its stream
      (first start .. last end, and the search's start after the first of them: a kernel's start is its dispatch, its
      workgroups may wait for CUs - that wait is what is read here as the delay between enqueue and start), its start
      against the end of the call's previous search (negative: it started that long before the previous one ended) and the
      overlap of the two on the device. Then, over the window of these calls: the time with no search kernel running at
      all, and the time with exactly one / two or more."""
import csv, sys


def load(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append({"s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]), "name": r["Kernel_Name"],
                         "thread": r.get("Thread_Id", "0"), "stream": r.get("Stream_Id", "0"), "queue": r.get("Queue_Id", "0"),
                         "id": int(r.get("Dispatch_Id", 0) or 0)})
    return rows


def short(n):
    if "plan_cost" in n: return "plan_cost"
    if "plan_rank" in n: return "plan_rank"
    if "plan_sort" in n: return "plan_sort"
    if "search_kernel" in n: return "search" + ("(streamed)" if n.rstrip(">) ").endswith("true") else "")
    return n[:40]


def plain(rows, last):
    rows = sorted((r["s"], r["e"], r["name"]) for r in rows)[-last:]
    t0 = rows[0][0]
    prev_end = None
    for s, e, n in rows:
        if prev_end is not None and s - prev_end > 50_000:
            t0 = s
            print("--")
        print("%9.1f .. %9.1f us  (%8.1f)  %s" % ((s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, short(n)))
        prev_end = max(prev_end or 0, e)


def calls_of(rows, chunks):
    """[(thread, [search launch dict with 'plans': the plan kernels ahead of it on its stream]...)] in order of first start"""
    calls = []
    by_thread = {}
    for r in sorted(rows, key=lambda r: r["id"]):
        if "search_kernel" in r["name"] or "plan_" in r["name"]:
            by_thread.setdefault(r["thread"], []).append(r)
    for th, rs in by_thread.items():
        pending, cur = [], []
        for r in rs:
            if "plan_" in r["name"]:
                pending.append(r)
                continue
            r = dict(r, plans=[p for p in pending if p["stream"] == r["stream"]])
            pending = []
            cur.append(r)
            if len(cur) == chunks:
                calls.append((th, cur))
                cur = []
    calls.sort(key=lambda c: min([x["s"] for x in c[1]] + [p["s"] for x in c[1] for p in x["plans"]]))
    return calls


def busy_levels(intervals, w0, w1):
    """time in [w0, w1) with 0, 1, >= 2 of the intervals open"""
    ev = []
    for s, e in intervals:
        s, e = max(s, w0), min(e, w1)
        if e > s:
            ev += [(s, 1), (e, -1)]
    ev.sort()
    lvl, t, out = 0, w0, [0, 0, 0]
    for x, d in ev:
        out[min(lvl, 2)] += x - t
        t = x
        lvl += d
    out[min(lvl, 2)] += w1 - t
    return out


def per_call(rows, n_calls, chunks):
    calls = calls_of(rows, chunks)[-n_calls:]
    threads = sorted({th for th, _ in calls})
    print("%d calls of %d search launches from %d host thread(s); us from the first kernel of the call" % (len(calls), chunks, len(threads)))
    print("call thr lane chunk |    start       end  duration | plan kernels: first start .. last end, search starts after | start - previous end  overlap")
    late, durs = [[] for _ in range(chunks)], [[] for _ in range(chunks)]
    plan_wait = []
    for ci, (th, ss) in enumerate(calls):
        t0 = min([x["s"] for x in ss] + [p["s"] for x in ss for p in x["plans"]])
        prev = None
        for j, x in enumerate(ss):
            u = lambda t: (t - t0) / 1e3   # noqa: E731
            if x["plans"]:
                p0, p1 = min(p["s"] for p in x["plans"]), max(p["e"] for p in x["plans"])
                pl = "%8.1f .. %8.1f  %8.1f" % (u(p0), u(p1), (x["s"] - p0) / 1e3)
                plan_wait.append((x["s"] - p0) / 1e3)
            else:
                pl = "%30s" % "none"
            if prev is None:
                rel = "%28s" % ""
            else:
                rel = "%12.1f  %12.1f" % ((x["s"] - prev["e"]) / 1e3, max(0, min(prev["e"], x["e"]) - x["s"]) / 1e3)
                late[j].append((x["s"] - prev["e"]) / 1e3)
            durs[j].append((x["e"] - x["s"]) / 1e3)
            print("%4d %3d %4s %5d | %8.1f  %8.1f  %8.1f | %s | %s" % (ci, threads.index(th), x["stream"], j, u(x["s"]), u(x["e"]),
                                                                       (x["e"] - x["s"]) / 1e3, pl, rel))
            prev = x
    searches = [(x["s"], x["e"]) for _, ss in calls for x in ss]
    w0, w1 = min(s for s, _ in searches), max(e for _, e in searches)
    lv = busy_levels(searches, w0, w1)
    n = len(calls)
    mean = lambda v: sum(v) / len(v) if v else float("nan")   # noqa: E731
    print("window of these calls: %.1f us = %.1f us per call" % ((w1 - w0) / 1e3, (w1 - w0) / 1e3 / n))
    print("no search kernel running: %.1f us (%.1f per call); exactly one: %.1f us (%.1f per call); two or more: %.1f us (%.1f per call)"
          % (lv[0] / 1e3, lv[0] / 1e3 / n, lv[1] / 1e3, lv[1] / 1e3 / n, lv[2] / 1e3, lv[2] / 1e3 / n))
    for j in range(chunks):
        print("chunk %d: mean duration %.1f us%s" % (j, mean(durs[j]), "" if not late[j] else
              "; starts %.1f us after the previous chunk's end on average (min %.1f, max %.1f)" % (mean(late[j]), min(late[j]), max(late[j]))))
    if plan_wait:
        print("searches behind plan kernels: %d; they start %.1f us after their first plan kernel on average (min %.1f, max %.1f)"
              % (len(plan_wait), mean(plan_wait), min(plan_wait), max(plan_wait)))
    else:
        print("searches behind plan kernels: 0")


if __name__ == "__main__":
    a = sys.argv[1:]
    rows = load(a[0])
    if "--calls" in a:
        k = int(a[a.index("--calls") + 1])
        c = int(a[a.index("--chunks") + 1]) if "--chunks" in a else 2
        per_call(rows, k, c)
    else:
        plain(rows, int(a[1]) if len(a) > 1 else 40)
