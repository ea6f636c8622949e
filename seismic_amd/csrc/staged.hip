// staged.hip — staged calls, the lean path behind sgpu_search / sgpu_batch_search: one pinned arena per lane, one H2D,
// the kernel, one D2H.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "device_index.hpp"
#include "filter.hpp"
#include "hip_util.hpp"
#include "launch_config.hpp"

namespace sgpu {

// ---- host-side breakdown of a staged call (tools/latency_probe.py, sgpu_search_sequential) ----
// A thread that sets call_timing() gets the wall time of every phase of its staged calls added up:
// [0] validate + launch plan  [1] staging (pinned arena)  [2] enqueue H2D  [3] configure + kernel launch
// [4] enqueue D2H  [5] wait for the stream  [6] copy the rows out
double*& call_timing() {
  static thread_local double* t = nullptr;
  return t;
}
static inline double now_us() {
  return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-3;
}
struct PhaseClock {
  double* acc;
  double t;
  PhaseClock() : acc(call_timing()), t(acc ? now_us() : 0.0) {}
  inline void lap(int i) {
    if (!acc) return;
    const double n = now_us();
    acc[i] += n - t;
    t = n;
  }
};

// How a call waits for its lane. hipStreamSynchronize parks the thread on an interrupt; waking it costs
// what the host's idle state costs (tens to hundreds of microseconds on a quiet box: VERDICT r02 #8 saw
// 192 us outside the kernel on the driver's box against 17 us on a busy one). A call small enough to be
// latency-bound polls the stream instead (hipStreamQuery, no system call once the signal is mapped)
// for at most SGPU_SPIN_US microseconds (default 2000) and only then parks. SGPU_WAIT=block|spin overrides.
// (done / done_seq: the launch stores done_seq into *done - pinned host memory - once every result row is there: the
// wait ends then, whether or not the launch itself has ended)
static hipError_t wait_lane(hipStream_t s, uint32_t nq, const volatile uint32_t* done = nullptr, uint32_t done_seq = 0) {
  // (both knobs are read through the per-call cache, like every other one: a test that flips them is not silently ignored)
  const char* wv = env_get("SGPU_WAIT");
  const int mode = (wv && !std::strcmp(wv, "block")) ? 0 : ((wv && !std::strcmp(wv, "spin")) ? 2 : 1);
  const double spin_us = (double)env_u32("SGPU_SPIN_US", 2000);
  if (mode == 2 || (mode == 1 && nq <= 256)) {
    const double t0 = now_us();
    for (;;) {
      if (done && __atomic_load_n((const uint32_t*)done, __ATOMIC_ACQUIRE) == done_seq) return hipSuccess;
      const hipError_t e = hipStreamQuery(s);
      if (e == hipSuccess) return hipSuccess;
      if (e != hipErrorNotReady) return e;
      if (now_us() - t0 > spin_us) break;
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#elif defined(__aarch64__)
      asm volatile("yield");
#endif
    }
  }
  return hipStreamSynchronize(s);
}

// Validates, plans, stages and launches one search of `nq` queries on `lane`: one H2D, the kernel, one
// D2H, all enqueued; staged_finish waits and hands the rows out. *slot is the lane's recycled batch.
// (q_base: the index of the first query in the caller's batch, for error messages.)
// (flt: the filter the chunk searches with - its view on this replica is fetched, built there on first use, once the
// queries have passed validation; null or flt->f null: unfiltered)
// (chunk: which launch of its call this is, 0 = the first or only one; followed: 2 = another chunk of the call comes
// behind it, 1 = other calls are in flight on the replica)
sgpu_status staged_launch(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                          const float* vals, uint32_t nq, uint32_t q_base, const sgpu_search_params& sp, sgpu_batch** slot,
                          uint32_t followed, const FilterRef* flt, uint32_t chunk) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (sp.k == 0) return fail(SGPU_EINVAL, "k must be > 0 (KHeap::new asserts, reference src/utils.rs:23)");
  if (sp.k > 1024) return fail(SGPU_ELIMIT, "k = %u exceeds the heap limit of 1024", sp.k);
  uint32_t max_nnz = 0;
  PhaseClock pc;
  env_refresh();
  // The offsets first (sizes, max_nnz); the components of a chunk whose plan the host computes right away - make_plan
  // indexes the index's arrays with them - and those of a device-planned chunk AFTER its H2D copy is enqueued: the pass
  // over the components (~50 us per 5000 queries) then runs while the copy does, ahead of the plan kernels and the search.
  if (!q_off || q_off[0] != 0) return fail(SGPU_EINVAL, "q_off[0] must be 0");
  sgpu_status st = validate_query_offsets(q_off, nq, q_base, &max_nnz);
  if (st != SGPU_OK) return st;
  if (q_off[nq] && (!comps || !vals)) return fail(SGPU_EINVAL, "null query arrays");
  bool validated = false;
  HIP_TRY(hipSetDevice(d->device));
  const uint64_t nnz = q_off[nq];
  const uint32_t k = sp.k;
  const sgpu_staged_arena A(nq, nnz, k);   // where everything lies in the lane's arena (device_index.hpp)
  sgpu_batch* b = *slot;
  if (b && (!b->staged || b->owner != d || b->arena_cap < A.total)) {
    HIP_TRY(hipStreamSynchronize(lane->stream));
    batch_free(b);
    b = nullptr;
    *slot = nullptr;
  }
  if (!b) {
    b = new (std::nothrow) sgpu_batch();
    if (!b) return fail(SGPU_ENOMEM, "out of host memory");
    b->staged = true;
    b->device = d->device;
    b->owner = d;
    // twice the need: a lane that has served one chunk of a call cut in four also holds a chunk of a call cut in two (the
    // number of chunks follows the load of the replica: cut_rule, call_cut.cpp) - no pinned reallocation in the middle of a stream of calls
    // (2.5 x: chunks of one call differ by a few per cent in components; the slack is bounded - the arena exists twice, in
    // HBM and as pinned host memory, per lane: ADVICE r05)
    b->arena_cap = std::max<size_t>(std::min<size_t>(A.total * 5 / 2, A.total + ((size_t)64 << 20)), 1 << 16);
    if (hipMalloc((void**)&b->arena_dev, b->arena_cap) != hipSuccess ||
        hipHostMalloc((void**)&b->arena_host, b->arena_cap, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {   // (fine-grained by request, not by the runtime's default: the kernel's rows and done word must be visible as they land)
      batch_free(b);
      return fail(SGPU_ENOMEM, "allocation of a %zu-byte staging arena failed", b->arena_cap);
    }
    if (hipHostGetDevicePointer((void**)&b->arena_host_dev, b->arena_host, 0) != hipSuccess) b->arena_host_dev = nullptr;
    *slot = b;
    if (hook_get("SGPU_DEBUG_ALLOC")) std::fprintf(stderr, "sgpu alloc: arena %p..%p\n", (void*)b->arena_dev, (void*)(b->arena_dev + b->arena_cap));
  }
  b->nq = nq;
  b->k_max = k;
  b->max_nnz = max_nnz;
  b->lay = A;
  b->q_base = q_base;
  if (nq == 0) {
    b->status_off = A.status;
    return SGPU_OK;
  }
  const uint32_t direct_max = hook_u32("SGPU_DIRECT_OUT_MAX", 16);   // (read per call: the knob cache is refreshed per call)
  const uint32_t cut = launch_cut(sp.query_cut, max_nnz);
  try {
    b->plans.clear();
    b->plans.emplace_back();
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory planning a query batch");
  }
  // The launch plan: on the DEVICE for chunks of 256 ... 16384 queries once a first chunk has told what this index and
  // query_cut need (r06, plan_kernel.hip: the calling thread no longer spends ~0.2 us per query on it - a third of a
  // one-thread call); on the host for small chunks (microseconds), for the first chunk, for a sorted first list (its
  // sort buffer must hold the chunk's largest first list: the host plan knows it exactly), for query_cut > 16 and for the
  // hashed lookup of u32 indexes (per-query seeds). SGPU_DEVICE_PLAN=0: always the host.
  // WHO PLANS WHICH CHUNK of a call that search_segment (abi.cpp, by the rules of call_cut.cpp) cut in several: chunk 0 goes out unplanned (below) with nothing ahead of
  // its search. A LATER chunk is planned here, on the calling thread, which would otherwise sit in its wait: the previous
  // chunk's persistent workgroups hold every CU until its queries run out, so plan kernels on this chunk's stream cannot
  // start before that tail (they completed 2.7 ms into a 10 000-query call) and the search behind them starts later still.
  // Host-planned, the chunk's order goes down with its copy and its search is queued, ready, long before the previous
  // search's first workgroup leaves; make_plan (~0.2 us per query) fits in the milliseconds that search takes. The device
  // plan stays where it pays: a call that is ONE launch has nothing to hide a host plan behind.
  // SGPU_CHUNK_PLAN=device: later chunks planned on the device too (the rule until this change; for A/B runs).
  b->device_plan_cut = 0xffffffffu;
  b->followed = followed != 0;
  b->plan_identity = false;
  {
    uint32_t seen = device_plan_dots(d, sp, nq, cut);
    if (seen && chunk > 0 && later_chunks_on_host()) seen = 0;
    if (seen && nq <= direct_max) seen = 0;   // (a call that small never copies its queries down: kDevicePlanMinQueries is far above, this is for the knob)
    if (!seen) {
      st = validate_queries(dim, q_off, comps, vals, nq, &max_nnz, q_base);
      if (st != SGPU_OK) return st;
      validated = true;
    }
    if (seen) {
      sgpu_batch_plan& pl = b->plans.back();
      pl.query_cut = cut;
      pl.dots_cap = std::max(seen, std::max<uint32_t>(d->max_nb, 1));
      pl.max_nb = 0;
      pl.max_list_nb = std::max<uint32_t>(d->max_nb, 1);   // (no list of the index has more blocks: a bound, not the chunk's maximum)
      pl.hash_ok = false;
      pl.order.clear();
      b->device_plan_cut = cut;
      // The chunk's own call sends another chunk right behind it: the order in which this one takes its queries decides
      // how long ITS tail is, and the next chunk's workgroups fill that tail whatever its length - the plan kernels (56 us
      // ahead of the first search workgroup of a call) are skipped, the queries are taken in input order (q_order = null),
      // and the LDS need of the index keeps coming from the chunks that are planned (SGPU_PLAN_IDENTITY=0, a test hook).
      b->plan_identity = followed == 2 && hook_u32("SGPU_PLAN_IDENTITY", 1) != 0;
    } else {
      st = make_plan(d, q_off, comps, vals, nq, cut, &b->plans.back());
      if (st != SGPU_OK) return st;
      // (the host plan sizes this chunk's LDS layout exactly; it also seeds and raises what device-planned chunks are sized
      // for - from chunks of the sizes the device plans only: a one-query latency call says nothing about a batch)
      if (nq >= kDevicePlanMinQueries) {
        std::lock_guard<std::mutex> lock(d->mu);
        uint32_t& v = d->plan_dots_seen[cut];
        v = std::max(v, b->plans.back().dots_cap);
      }
    }
  }
  pc.lap(0);
  uint8_t* hs = b->arena_host;
  std::memset(hs, 0, 16);
  uint32_t* h32 = (uint32_t*)(hs + A.off);
  for (uint32_t q = 0; q <= nq; ++q) h32[q] = (uint32_t)q_off[q];
  if (nnz) {
    std::memcpy(hs + A.comp, comps, nnz * 4);
    std::memcpy(hs + A.val, vals, nnz * 4);
  }
  if (b->device_plan_cut == 0xffffffffu) std::memcpy(hs + A.order, b->plans.back().order.data(), (size_t)nq * 8);
  std::memset(hs + A.status, 0, 16);
  std::memset(hs + A.fix, 0, 16);
  // A latency-bound call (a handful of queries) has the kernel write its few result rows straight into the pinned
  // host arena (mapped, fine-grained: posted writes over PCIe, visible once the stream is done): no D2H copy to
  // enqueue, none to wait for. Larger calls keep the device-side slab and one D2H. Since r04 such a call also lets the
  // kernel READ its queries (a few hundred bytes) from that arena: no H2D copy to enqueue (5 us of host time and a
  // copy command ahead of the kernel) - which leaves the work counter: it is not zeroed per launch but runs on
  // (KParams::queue_base; Lane::queue_pos mirrors it on the host).
  const uint32_t direct_in_on = env_u32("SGPU_DIRECT_IN", 1);
  b->direct_out = b->arena_host_dev != nullptr && nq <= direct_max;
  b->direct_in = b->direct_out && direct_in_on != 0;
  uint8_t* in_base = b->direct_in ? b->arena_host_dev : b->arena_dev;
  b->queue_dev = b->direct_in ? lane->queue + 16 : (uint32_t*)b->arena_dev;
  b->queue_base = 0;
  b->q_off = (uint32_t*)(in_base + A.off);
  b->q_comp = (uint32_t*)(in_base + A.comp);
  b->q_val = (float*)(in_base + A.val);
  b->q_order = (uint32_t*)(in_base + A.order);
  b->order_cut = cut;
  uint8_t* out_base = b->direct_out ? b->arena_host_dev : b->arena_dev;
  b->out_n = (uint32_t*)(out_base + A.out_n);
  b->out_scores = (float*)(out_base + A.out_scores);
  b->out_ids = (uint64_t*)(out_base + A.out_ids);
  b->out_stats = nullptr;
  b->status_off = b->direct_out ? A.fix : A.status;
  b->status = (uint32_t*)(out_base + b->status_off);
  pc.lap(1);
  if (b->direct_in) {
    if (lane->queue_dirty) {   // first use of the lane, or a launch on it failed: the counter's value is not known
      HIP_TRY(hipMemsetAsync(lane->queue + 16, 0, 4, lane->stream));
      lane->queue_pos = 0;
      lane->queue_dirty = false;
    }
    b->queue_base = lane->queue_pos;
  } else {
    HIP_TRY(hipMemcpyAsync(b->arena_dev, hs, A.in_bytes, hipMemcpyHostToDevice, lane->stream));
    if (!validated) {   // (the copy is on its way: nothing that reads the components has been enqueued yet)
      st = validate_queries(dim, q_off, comps, vals, nq, &max_nnz, q_base);
      if (st != SGPU_OK) {
        const std::string msg = last_error();
        (void)hipStreamSynchronize(lane->stream);
        last_error() = msg;
        return st;
      }
      validated = true;
    }
  }
  const DevView* view = &d->view;
  if (flt && flt->f) {   // (the queries are valid: a filtered call fails as the unfiltered one would up to here)
    const FilterDeviceView* fv = nullptr;
    st = filter_view(flt->f, flt->replica, &fv);
    if (st != SGPU_OK) {
      const std::string msg = last_error();
      (void)hipStreamSynchronize(lane->stream);
      last_error() = msg;
      return st;
    }
    view = &fv->view;
    HIP_TRY(hipSetDevice(d->device));
  }
  if (!b->direct_in && b->device_plan_cut != 0xffffffffu && !b->plan_identity) {
    // order -> the arena's order region; the maxima -> words 1 - 3 of the status block (zeroed by the copy above, they
    // come back with the rows); the sort keys borrow the output region, which the search kernel overwrites afterwards
    // (16 bytes per query at least: room for the <= 2 nq keys)
    HIP_TRY(launch_device_plan(*view, b->q_off, b->q_comp, b->q_val, nq, cut, (uint64_t*)(b->arena_dev + A.out_n),
                               (uint32_t*)(b->arena_dev + A.status) + 1, b->q_order, lane->stream));
  }
  pc.lap(2);
  // from here on a failure waits for the stream: the lane (and its pinned arena) goes back to the pool
  hipError_t he = hipSuccess;
  {
    std::lock_guard<std::mutex> lock(d->mu);   // the occupancy cache is shared by the lanes
    LaunchArgs a{};
    st = configure(d, lane, b, sp, MODE_SEARCH, &a, view);
    if (st == SGPU_OK) he = launch_search(a);
    if (st == SGPU_OK && he == hipSuccess) lane->variant_commit();
    if (b->direct_in) {
      if (st == SGPU_OK && he == hipSuccess) lane->queue_pos += nq + a.grid;   // the tickets this launch takes
      else lane->queue_dirty = true;
    }
  }
  pc.lap(3);
  if (st == SGPU_OK && he == hipSuccess && !b->direct_out)
    he = hipMemcpyAsync(hs + A.status, b->arena_dev + A.status, A.total - A.status, hipMemcpyDeviceToHost, lane->stream);
  pc.lap(4);
  if (st != SGPU_OK || he != hipSuccess) {
    (void)hipStreamSynchronize(lane->stream);
    if (st == SGPU_OK) st = fail(SGPU_EDEVICE, "launch of the search failed: %s", hipGetErrorString(he));
    return st;
  }
  return SGPU_OK;
}

// (test hook: the last chunk pool lane `lane` served - info4 = {queries, first query in its call's batch, who planned it:
// 0 the host / 1 the device / 2 nobody (input order), query_cut} - and, host-planned, the order that went down with its
// queries, as staged in the pinned arena. Returns 0 where the lane has served nothing. sgpu_debug_lane_chunk)
uint32_t debug_lane_chunk(DeviceIndex* d, uint32_t lane, uint32_t* info4, uint32_t* order_out, uint32_t cap) {
  if (!d || lane >= (uint32_t)DeviceIndex::kPool) return 0;
  std::lock_guard<std::mutex> lk(d->pool_mu);
  const Lane& l = d->pool[lane];
  const sgpu_batch* b = l.scratch;
  if (l.busy || !b || !b->staged || b->nq == 0) return 0;
  const bool host = b->device_plan_cut == 0xffffffffu;
  info4[0] = b->nq;
  info4[1] = b->q_base;
  info4[2] = host ? 0u : (b->plan_identity ? 2u : 1u);
  info4[3] = b->order_cut;
  if (host && order_out) std::memcpy(order_out, b->arena_host + b->lay.order, (size_t)std::min<uint32_t>(cap, b->nq) * 4);
  return 1;
}

// Waits for the lane's staged search and copies the rows out (nq x k slabs, row q padded past out_n[q]).
sgpu_status staged_finish(DeviceIndex* d, Lane* lane, sgpu_batch* b, float* out_scores, uint64_t* out_ids, uint32_t* out_n) {
  HIP_TRY(hipSetDevice(d->device));
  PhaseClock pc;
  {
    const volatile uint32_t* done = (b && b->done_seq) ? (const volatile uint32_t*)(b->arena_host + b->status_off + 4) : nullptr;
    const hipError_t we = wait_lane(lane->stream, b ? b->nq : 0, done, b ? b->done_seq : 0u);
    if (we != hipSuccess) lane->queue_dirty = true;   // (the running work counter of direct-in calls is no longer known)
    HIP_TRY(we);
  }
  pc.lap(5);
  if (!b || b->nq == 0) return SGPU_OK;
  {   // the launch's status word came back with the rows (cooperative protocol errors, bounded waits of the streamed variant)
    const sgpu_status cs = coop_report(d, lane, *(const volatile uint32_t*)(b->arena_host + b->status_off));
    if (cs != SGPU_OK) {
      lane->queue_dirty = true;
      return cs;
    }
  }
  if (b->device_plan_cut != 0xffffffffu) {   // what this chunk's queries needed: the next chunks' LDS layouts are sized for it
    const uint32_t need = ((const volatile uint32_t*)(b->arena_host + b->status_off))[1];
    std::lock_guard<std::mutex> lock(d->mu);
    uint32_t& v = d->plan_dots_seen[b->device_plan_cut];
    v = std::max(v, need);
  }
  const size_t nq = b->nq, k = b->k_max;
  std::memcpy(out_n, b->arena_host + b->lay.out_n, nq * 4);
  std::memcpy(out_scores, b->arena_host + b->lay.out_scores, nq * k * 4);
  std::memcpy(out_ids, b->arena_host + b->lay.out_ids, nq * k * 8);
  pc.lap(6);
  return SGPU_OK;
}

}  // namespace sgpu
