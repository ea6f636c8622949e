// batch.hip — device-resident query batches (sgpu_batch_*): create, configure and launch a search pass, fetch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_index.hpp"
#include "hip_util.hpp"
#include "launch_config.hpp"

namespace sgpu {

// one translation unit per kernel family (sk_*.hip): occupancy query when `occupancy` is given, else launch
hipError_t run_u16_dense(const LaunchArgs& a, int* occupancy);
hipError_t run_u16_packed(const LaunchArgs& a, int* occupancy);
hipError_t run_u32_split(const LaunchArgs& a, int* occupancy);
hipError_t run_u32_packed(const LaunchArgs& a, int* occupancy);
hipError_t run_u32_hash(const LaunchArgs& a, int* occupancy);
hipError_t run_u16_dense_u8(const LaunchArgs& a, int* occupancy);
hipError_t run_u16_packed_u8(const LaunchArgs& a, int* occupancy);
hipError_t run_u32_packed_u8(const LaunchArgs& a, int* occupancy);
hipError_t run_u32_split_u8(const LaunchArgs& a, int* occupancy);
hipError_t run_u16_dense_dvb(const LaunchArgs& a, int* occupancy);
hipError_t run_u16_packed_dvb(const LaunchArgs& a, int* occupancy);

static hipError_t run_any(const LaunchArgs& a, int* occ) {
  // (u16 components: dense byte table or packed {bits, rank} words. The hashed lookup is the u32 layout: for u16 it
  // measured slower than both - 6.46 against 5.81 ms per 10 000-query launch, profiles/r03_lds_sensitivity.md - and its
  // three families were dropped in r05)
  if (a.comp_width == 2 && a.lookup != LK_DENSE && a.lookup != LK_PACKED) return hipErrorInvalidConfiguration;
  if (a.value_type == SGPU_VAL_DOTVBYTE)   // (u16 components only)
    return a.lookup == LK_DENSE ? run_u16_dense_dvb(a, occ) : run_u16_packed_dvb(a, occ);
  if (a.value_type == SGPU_VAL_FIXEDU8 && a.comp_width == 4) return a.lookup == LK_SPLIT ? run_u32_split_u8(a, occ) : run_u32_packed_u8(a, occ);
  if (a.value_type == SGPU_VAL_FIXEDU8) return a.lookup == LK_DENSE ? run_u16_dense_u8(a, occ) : run_u16_packed_u8(a, occ);
  if (a.comp_width == 2) return a.lookup == LK_DENSE ? run_u16_dense(a, occ) : run_u16_packed(a, occ);
  if (a.lookup == LK_HASH) return run_u32_hash(a, occ);
  return a.lookup == LK_SPLIT ? run_u32_split(a, occ) : run_u32_packed(a, occ);
}
hipError_t occupancy_search(const LaunchArgs& a, int* blocks_per_cu) { return run_any(a, blocks_per_cu); }
hipError_t launch_search(const LaunchArgs& a) { return run_any(a, nullptr); }

void batch_free(sgpu_batch* b) {
  if (!b) return;
  if (b->device >= 0) (void)hipSetDevice(b->device);
  if (b->staged) {
    (void)hipFree(b->arena_dev);
    (void)hipHostFree(b->arena_host);
    delete b;
    return;
  }
  (void)hipFree(b->q_off);
  (void)hipFree(b->q_comp);
  (void)hipFree(b->q_val);
  (void)hipFree(b->q_order);
  (void)hipHostFree(b->h_order);
  (void)hipFree(b->out_scores);
  (void)hipFree(b->out_ids);
  (void)hipFree(b->out_n);
  (void)hipFree(b->out_stats);
  delete b;
}

// Creates (or, when *out already holds a large enough batch of the same device, refills) a device
// batch. The copies are enqueued on `lane`'s stream from the batch's own host copies of the arrays;
// the caller's buffers are not referenced after the call returns.
sgpu_status batch_create(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                         const float* vals, uint32_t nq, uint32_t k_max, sgpu_batch** out) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (k_max == 0) return fail(SGPU_EINVAL, "k == 0");
  if (k_max > 1024) return fail(SGPU_ELIMIT, "k = %u exceeds the heap limit of 1024", k_max);
  uint32_t max_nnz = 0;
  sgpu_status st = validate_queries(dim, q_off, comps, vals, nq, &max_nnz);
  if (st != SGPU_OK) return st;
  HIP_TRY(hipSetDevice(d->device));
  const uint64_t nnz = q_off[nq];
  const size_t slab = std::max<size_t>((size_t)nq * k_max, 1);
  sgpu_batch* b = *out;
  const bool reuse = b && b->owner == d && b->cap_nq >= nq && b->cap_nnz >= nnz && b->cap_slab >= slab;
  if (b && !reuse) {
    HIP_TRY(hipStreamSynchronize(lane->stream));
    batch_free(b);
    b = nullptr;
    *out = nullptr;
  }
  if (reuse) HIP_TRY(hipStreamSynchronize(lane->stream));   // earlier copies out of the batch's host arrays are done
  try {
    if (!b) b = new sgpu_batch();
    b->device = d->device;
    b->owner = d;
    b->nq = nq;
    b->k_max = k_max;
    b->max_nnz = max_nnz;
    b->plans.clear();
    b->order_cut = 0xffffffffu;
    b->h_off.assign(q_off, q_off + nq + 1);
    b->h_comp.assign(comps, comps + nnz);
    b->h_val.assign(vals, vals + nnz);
    b->h_off32.resize((size_t)nq + 1);
  } catch (const std::bad_alloc&) {
    if (!reuse) delete b;
    else b->nq = 0;   // the recycled batch stays valid, and empty
    return fail(SGPU_ENOMEM, "out of host memory creating a query batch");
  }
  for (uint32_t q = 0; q <= nq; ++q) b->h_off32[q] = (uint32_t)q_off[q];
  bool ok = true;
  if (!reuse) {
    // a recycled batch grows geometrically so that a stream of slightly different calls settles
    b->cap_nq = std::max<uint64_t>(nq, 1);
    b->cap_nnz = std::max<uint64_t>(nnz, 1);
    b->cap_slab = slab;
    ok = hipMalloc((void**)&b->q_off, (b->cap_nq + 1) * 4) == hipSuccess &&
         hipMalloc((void**)&b->q_comp, b->cap_nnz * 4) == hipSuccess &&
         hipMalloc((void**)&b->q_val, b->cap_nnz * 4) == hipSuccess &&
         hipMalloc((void**)&b->q_order, b->cap_nq * 8) == hipSuccess &&
         hipHostMalloc((void**)&b->h_order, b->cap_nq * 8, hipHostMallocDefault) == hipSuccess &&
         hipMalloc((void**)&b->out_scores, std::max<size_t>(slab, 65536) * 4) == hipSuccess &&
         hipMalloc((void**)&b->out_ids, slab * 8) == hipSuccess &&
         hipMalloc((void**)&b->out_n, b->cap_nq * 4) == hipSuccess &&
         hipMalloc((void**)&b->out_stats, b->cap_nq * STATS_WORDS * 4) == hipSuccess;
  }
  if (!ok) {
    batch_free(b);
    *out = nullptr;
    return fail(SGPU_ENOMEM, "hipMalloc failed creating a query batch");
  }
  ok = hipMemcpyAsync(b->q_off, b->h_off32.data(), (nq + 1) * 4, hipMemcpyHostToDevice, lane->stream) == hipSuccess &&
       (nnz == 0 ||
        (hipMemcpyAsync(b->q_comp, b->h_comp.data(), nnz * 4, hipMemcpyHostToDevice, lane->stream) == hipSuccess &&
         hipMemcpyAsync(b->q_val, b->h_val.data(), nnz * 4, hipMemcpyHostToDevice, lane->stream) == hipSuccess));
  if (!ok) {
    (void)hipStreamSynchronize(lane->stream);
    batch_free(b);
    *out = nullptr;
    return fail(SGPU_EDEVICE, "hipMemcpy of the query batch failed");
  }
  *out = b;
  return SGPU_OK;
}

const DeviceIndex* batch_replica(const sgpu_batch* b) { return b ? b->owner : nullptr; }

// One search pass: launch_configure (launch_config.cpp) decides everything a pure function can; what is left here touches
// the device or the lane - the plan, the order's staging copy, the pointers, the occupancy cache, board and bitmaps.
sgpu_status configure(DeviceIndex* d, Lane* lane, sgpu_batch* b, const sgpu_search_params& sp, uint32_t mode, LaunchArgs* a,
                      const DevView* ov) {
  const Knobs& kn = launch_knobs();
  LaunchInput in;
  in.n_cu = d->n_cu, in.max_lds = d->max_lds, in.comp_width = d->comp_width, in.value_type = d->value_type, in.dim = d->view.dim;
  in.val_scale = d->val_scale, in.coop_broken = d->coop_broken;
  in.nq = b->nq, in.max_nnz = b->max_nnz, in.k_max = b->k_max, in.staged = b->staged, in.queue_base = b->queue_base;
  in.sp = sp, in.mode = mode, in.knobs = kn;
  const uint32_t cut = mode == MODE_DOTS ? 1u : launch_cut(sp.query_cut, b->max_nnz);
  const sgpu_batch_plan* pl = nullptr;
  if (mode == MODE_DOTS) {
    in.target_list_nb = d->list_nb[sp.query_cut];
  } else if (sp.k != 0 && sp.k <= b->k_max) {   // (else: launch_configure fails the call before it looks at a plan)
    sgpu_status pst = plan_for(d, b, cut, &pl);
    if (pst != SGPU_OK) return pst;
    in.has_plan = true, in.dots_cap = pl->dots_cap, in.max_nb = pl->max_nb, in.max_list_nb = pl->max_list_nb, in.hash_ok = pl->hash_ok;
  }
  LaunchConfig c;
  sgpu_status cst = launch_configure(in, &c);
  if (cst != SGPU_OK) return cst;
  a->L = c.L;
  a->p = c.p;
  a->lookup = c.lookup;
  a->counted = c.counted;
  a->streamed = c.streamed;
  a->value_type = d->value_type;
  a->ix = ov ? *ov : d->view;
  a->comp_width = d->comp_width;
  a->block = c.block;
  a->lds_bytes = c.lds_bytes;
  if (kn.debug)
    std::fprintf(stderr, "sgpu configure: nq %u NT %u lookup %u items_max %u ring %u dots_cap %u lists/group %u of %u uni %llu lds %llu\n", b->nq, c.block, c.lookup,
                 c.p.items_max, c.ring, c.L.dots_cap, c.L.qg, c.L.qc, (unsigned long long)(c.lds_bytes - c.L.uni), (unsigned long long)c.lds_bytes);
  a->stream = lane->stream;
  a->qb.q_off = b->q_off;
  a->qb.q_comp = b->q_comp;
  a->qb.q_val = b->q_val;
  a->qb.nq = b->nq;
  a->qb.k_stride = b->k_max;
  a->qb.out_scores = b->out_scores;
  a->qb.out_ids = b->out_ids;
  a->qb.out_n = b->out_n;
  a->qb.q_order = nullptr;
  a->qb.q_seed = nullptr;
  if (pl && !kn.no_lpt && b->nq && !b->plan_identity) {
    // the processing order lives in the batch's own device buffer (no allocation on the path)
    if (b->order_cut != cut) {
      if (b->order_cut != 0xffffffffu) HIP_TRY(hipStreamSynchronize(lane->stream));   // the staging copy may be in flight
      std::memcpy(b->h_order, pl->order.data(), (size_t)b->nq * 8);   // [order | hash seeds]
      HIP_TRY(hipMemcpyAsync(b->q_order, b->h_order, (size_t)b->nq * 8, hipMemcpyHostToDevice, lane->stream));
      b->order_cut = cut;
    }
    a->qb.q_order = b->q_order;
    a->qb.q_seed = b->q_order + b->nq;
  }
  a->qb.out_stats = mode != MODE_DOTS ? b->out_stats : nullptr;   // (null for staged batches: no work counters)
  // launch status word: a staged batch's travels back with its rows; a device-resident batch uses the lane's sticky word
  // (queue + 32, zero from lane_init on; read after the rows by batch_fetch / batch_sync)
  a->qb.status = b->staged ? b->status : lane->queue + 32;
  a->qb.done = nullptr;   // (set below for cooperative launches that write their rows to the host arena)
  a->qb.done_seq = 0;
  // occupancy of this kernel variant at this LDS size: queried once, then remembered
  a->coop = CoopView{};
  a->coop.enabled = c.coop != 0;   // (the cooperative variant is its own kernel symbol)
  int per_cu = 0;
  {
    const uint64_t key = ((uint64_t)(a->streamed != 0) << 59) | ((uint64_t)(a->coop.enabled != 0) << 58) | ((uint64_t)a->comp_width << 56) | ((uint64_t)a->counted << 55) | ((uint64_t)a->value_type << 52) | ((uint64_t)a->block << 40) | ((uint64_t)a->lookup << 36) |
                         ((uint64_t)heap_variant(a->p.k) << 28) | (uint64_t)(a->lds_bytes >> 4);
    auto it = d->occupancy.find(key);
    if (it == d->occupancy.end()) {
      HIP_TRY(occupancy_search(*a, &per_cu));
      d->occupancy[key] = per_cu;
    } else {
      per_cu = it->second;
    }
  }
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the search kernel does not fit on a CU with %llu bytes of LDS", (unsigned long long)c.lds_bytes);
  if (kn.wg_per_cu && (uint32_t)per_cu > kn.wg_per_cu) per_cu = (int)kn.wg_per_cu;
  uint32_t uncapped = 0;
  const uint32_t grid = launch_grid(c, b->nq, d->n_cu * (uint32_t)per_cu, &uncapped);
  if (uncapped > grid && kn.debug) std::fprintf(stderr, "sgpu coop: grid %u capped at 512 (board size)\n", uncapped);
  if (c.coop) {
    // every slot of the grid is launched, workgroups without a query help the ones that own one: their board
    CoopView& v = a->coop;
    v.max_pos = c.max_pos, v.max_cand = c.max_cand, v.chunk = c.chunk, v.chunk_min = c.chunk_min, v.min_items = c.min_items;
    v.first_reach = c.first_reach, v.idle_min = c.idle_min, v.idle_ratio = c.idle_ratio, v.poll_sleep = c.poll_sleep;
    const CoopBoard bd = coop_board(grid, c.max_pos, c.max_cand);
    if (lane->coop_bytes < bd.total) {
      if (lane->coop) {
        HIP_TRY(hipStreamSynchronize(lane->stream));
        (void)hipFree(lane->coop);
      }
      lane->coop = nullptr;
      lane->coop_bytes = 0;
      if (hipMalloc((void**)&lane->coop, bd.total) != hipSuccess)
        return fail(SGPU_ENOMEM, "hipMalloc of the %zu-byte cooperative board failed", bd.total);
      lane->coop_bytes = bd.total;
      HIP_TRY(hipMemsetAsync(lane->coop, 0, bd.total, lane->stream));
    } else if (lane->coop_bytes && kn.coop_reset) {   // (debugging aid: do not trust the kernel's own clean-up)
      HIP_TRY(hipMemsetAsync(lane->coop, 0, bd.pos, lane->stream));
    }
    if (kn.debug)
      std::fprintf(stderr, "sgpu coop: board %p..%p slots@%zu pos@%zu cand@%zu grid %u max_pos %u max_cand %u chunk %u..%u min_items %u idle_min %u idle_ratio %u\n",
                   (void*)lane->coop, (void*)(lane->coop + bd.total), bd.slots, bd.pos, bd.cand, grid, v.max_pos, v.max_cand, v.chunk_min, v.chunk,
                   v.min_items, v.idle_min, v.idle_ratio);
    v.open = (uint64_t*)lane->coop;
    v.counters = (uint32_t*)(lane->coop + 64);
    v.slots = (uint64_t*)(lane->coop + bd.slots);
    v.pos_pub = (uint64_t*)(lane->coop + bd.pos);
    v.cands = (uint64_t*)(lane->coop + bd.cand);
    v.trace = nullptr;
    if (kn.coop_trace) {   // (trace builds) the timeline of this launch: zeroed here, dumped by coop_trace_dump
      v.trace = (uint64_t*)(lane->coop + bd.trace);
      HIP_TRY(hipMemsetAsync(lane->coop + bd.trace, 0, (size_t)grid * 16 * 8, lane->stream));
      lane->coop_trace_off = bd.trace;
      lane->coop_trace_n = grid * 16;
    }
  }
  a->grid = grid;
  // A cooperative launch that writes its rows straight into the pinned host arena also tells the host when the LAST
  // query's rows are there (BatchView::done): the call returns them while the launch winds down (helpers leaving, the
  // board being cleared), and the next call's launch queues up behind it (r04; SGPU_EARLY_DONE=0: wait for the launch).
  b->done_seq = 0;
  if (a->coop.enabled && b->staged && b->direct_out && b->status && kn.early_done) {
    lane->done_seq = lane->done_seq == 0xffffffffu ? 1u : lane->done_seq + 1u;
    b->done_seq = lane->done_seq;
    a->qb.done = b->status + 1;
    a->qb.done_seq = b->done_seq;
  }
  // visited bitmaps: one per resident workgroup (counted pass)
  a->bitmaps = nullptr;
  if (a->counted) {
    if (lane->bitmaps_slots < grid) {
      if (lane->bitmaps) {
        HIP_TRY(hipStreamSynchronize(lane->stream));
        (void)hipFree(lane->bitmaps);
      }
      lane->bitmaps = nullptr;
      lane->bitmaps_slots = 0;
      const uint32_t slots = std::max<uint32_t>(grid, d->n_cu * (uint32_t)per_cu);
      const size_t bytes = (size_t)slots * std::max<uint32_t>(d->view.n_bitmap_words, 1) * 4;
      if (hipMalloc((void**)&lane->bitmaps, bytes) != hipSuccess)
        return fail(SGPU_ENOMEM, "hipMalloc of %zu bytes of visited bitmaps failed", bytes);
      HIP_TRY(hipMemsetAsync(lane->bitmaps, 0, bytes, lane->stream));
      lane->bitmaps_slots = slots;
    }
    a->bitmaps = lane->bitmaps;
  }
  a->queue = b->staged ? b->queue_dev : lane->queue;
  lane->coop_last = a->coop.enabled != 0;
  lane->variant_next[0] = c.lookup, lane->variant_next[1] = c.streamed, lane->variant_next[2] = c.coop, lane->variant_next[3] = c.counted;
  return SGPU_OK;
}

// (test hook: the kernel variant of the last search launch of a lane of replica d - the main lane, which the resident batch
// API runs on, for lane < 0, else chunk pool lane `lane` - out4 = {lookup, streamed, cooperative 0 / 1 / 2 forced, counted}.
// Recorded next to lane->last once the launch has gone out; a dots launch (summary_distances) does not touch it. Returns 0
// where the lane has launched no search or is serving a call. sgpu_debug_lane_variant)
uint32_t debug_lane_variant(DeviceIndex* d, int32_t lane, uint32_t* out4) {
  if (!d || !out4 || lane >= (int32_t)DeviceIndex::kPool) return 0;
  const Lane* l = lane < 0 ? &d->main : &d->pool[lane];
  if (lane >= 0) {
    std::lock_guard<std::mutex> pool(d->pool_mu);
    if (l->busy) return 0;
  }
  std::lock_guard<std::mutex> lock(d->mu);   // (configure writes the words under it)
  if (!l->variant_set) return 0;
  std::memcpy(out4, l->variant, sizeof(l->variant));
  return 1;
}

static void drain_events(Lane* l) {   // stream must be idle
  for (int i = 0; i < l->ev_pending; ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, l->ev0[i], l->ev1[i]) == hipSuccess) {
      l->sum_ms += ms;
      l->n_timed += 1;
    }
  }
  l->ev_pending = 0;
}

// A cooperative launch that met a protocol error (a bounded device-side wait that gave up, control words of the
// wrong round) says so in its status word / the board's sticky word. EVERY cooperative launch is checked (r03 did
// so only under SGPU_COOP_CHECK): the call fails loudly, the sticky word is cleared so that later calls are
// judged on their own, and the variant stays off for this replica from then on (plain launches carry on).
sgpu_status coop_report(DeviceIndex* d, Lane* lane, uint32_t code) {
  if (!code) return SGPU_OK;
  if (code >= 16) {   // streamed stage 2: a bounded wait of a role gave up (16 replayer, 17 feeder, 18 scorer)
    (void)hipStreamSynchronize(lane->stream);
    return fail(SGPU_EDEVICE, "search kernel (streamed stage 2): a bounded wait gave up (code %u)", code);
  }
  if (lane->coop) (void)hipMemsetAsync(lane->coop + 64 + 12, 0, 4, lane->stream);
  (void)hipStreamSynchronize(lane->stream);
  if (!d->coop_broken) std::fprintf(stderr, "seismic_hip: cooperative search kernel reported protocol error %u on device %d; "
                                            "the cooperative variant is switched off for this index replica\n", code, d->device);
  d->coop_broken = true;
  return fail(SGPU_EDEVICE, "cooperative search kernel: protocol wait gave up (code %u)", code);
}
static sgpu_status coop_check_board(DeviceIndex* d, Lane* lane) {   // device-resident batches (not the latency path)
  uint32_t flag = 0;
  HIP_TRY(hipMemcpy(&flag, lane->queue + 32, 4, hipMemcpyDeviceToHost));   // the lane's sticky status word (streamed variants)
  if (flag) {
    (void)hipMemset(lane->queue + 32, 0, 4);
    return coop_report(d, lane, flag);
  }
  if (!lane->coop || !lane->coop_last) return SGPU_OK;
  HIP_TRY(hipMemcpy(&flag, lane->coop + 64 + 12, 4, hipMemcpyDeviceToHost));
  return coop_report(d, lane, flag);
}

// Enqueues one pass on `lane` (the index's main lane when null).
sgpu_status batch_run(DeviceIndex* d, Lane* lane, sgpu_batch* b, const sgpu_search_params& sp, uint32_t mode,
                      int sync, sgpu_launch_stats* stats) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (!b || b->owner != d) return fail(SGPU_EINVAL, "batch does not belong to this index replica");
  if (!lane) lane = &d->main;
  HIP_TRY(hipSetDevice(d->device));
  if (b->nq == 0) {
    if (stats) *stats = sgpu_launch_stats{};
    return SGPU_OK;
  }
  env_refresh();
  {
    // configuration touches state shared by the lanes (occupancy cache, bitmaps); a main-lane
    // launch also owns the main lane's event ring
    std::lock_guard<std::mutex> lock(d->mu);
    LaunchArgs a{};
    sgpu_status st = configure(d, lane, b, sp, mode, &a);
    if (st != SGPU_OK) return st;
    if (lane->ev_pending == (int)lane->ev0.size()) {
      HIP_TRY(hipStreamSynchronize(lane->stream));
      drain_events(lane);
    }
    HIP_TRY(hipMemsetAsync(lane->queue, 0, 4, lane->stream));
    if (a.qb.out_stats) HIP_TRY(hipMemsetAsync(b->out_stats, 0, (size_t)b->nq * STATS_WORDS * 4, lane->stream));
    const int e = lane->ev_pending++;
    HIP_TRY(hipEventRecord(lane->ev0[e], lane->stream));
    HIP_TRY(launch_search(a));
    HIP_TRY(hipEventRecord(lane->ev1[e], lane->stream));
    lane->last.n_queries = b->nq;
    lane->last.grid = a.grid;
    lane->last.block = a.block;
    lane->last.lds_bytes = a.lds_bytes;
    if (mode != MODE_DOTS) lane->variant_commit();
  }
  if (sync) {
    HIP_TRY(hipStreamSynchronize(lane->stream));
    std::lock_guard<std::mutex> lock(d->mu);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, lane->ev0[lane->ev_pending - 1], lane->ev1[lane->ev_pending - 1]));
    drain_events(lane);
    lane->last.kernel_ms = ms;
    if (stats) *stats = lane->last;
  }
  return SGPU_OK;
}

// Waits for everything enqueued on the main lane; stats->kernel_ms = mean kernel duration since the last sync.
sgpu_status batch_sync(DeviceIndex* d, sgpu_launch_stats* stats) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device");
  Lane* l = &d->main;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipStreamSynchronize(l->stream));
  std::lock_guard<std::mutex> lock(d->mu);
  drain_events(l);
  if (stats) {
    *stats = l->last;
    stats->kernel_ms = l->n_timed ? (float)(l->sum_ms / l->n_timed) : 0.0f;
  }
  l->sum_ms = 0;
  l->n_timed = 0;
  return SGPU_OK;
}

sgpu_status batch_fetch(DeviceIndex* d, Lane* lane, sgpu_batch* b, uint32_t k, float* out_scores, uint64_t* out_ids,
                        uint32_t* out_n) {
  if (!d || !b) return fail(SGPU_EINVAL, "null index/batch");
  if (k == 0 || k > b->k_max) return fail(SGPU_EINVAL, "k out of range for this batch");
  if (!lane) lane = &d->main;
  HIP_TRY(hipSetDevice(d->device));
  if (b->nq == 0) {
    HIP_TRY(hipStreamSynchronize(lane->stream));
    return SGPU_OK;
  }
  if (k == b->k_max) {
    HIP_TRY(hipMemcpyAsync(out_scores, b->out_scores, (size_t)b->nq * k * 4, hipMemcpyDeviceToHost, lane->stream));
    HIP_TRY(hipMemcpyAsync(out_ids, b->out_ids, (size_t)b->nq * k * 8, hipMemcpyDeviceToHost, lane->stream));
  } else {
    HIP_TRY(hipMemcpy2DAsync(out_scores, (size_t)k * 4, b->out_scores, (size_t)b->k_max * 4, (size_t)k * 4, b->nq,
                             hipMemcpyDeviceToHost, lane->stream));
    HIP_TRY(hipMemcpy2DAsync(out_ids, (size_t)k * 8, b->out_ids, (size_t)b->k_max * 8, (size_t)k * 8, b->nq,
                             hipMemcpyDeviceToHost, lane->stream));
  }
  HIP_TRY(hipMemcpyAsync(out_n, b->out_n, (size_t)b->nq * 4, hipMemcpyDeviceToHost, lane->stream));
  HIP_TRY(hipStreamSynchronize(lane->stream));
  return coop_check_board(d, lane);
}

sgpu_status batch_fetch_stats(DeviceIndex* d, sgpu_batch* b, uint32_t* out) {
  if (!d || !b || !out) return fail(SGPU_EINVAL, "null index/batch/out");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipStreamSynchronize(d->main.stream));
  if (b->nq) HIP_TRY(hipMemcpy(out, b->out_stats, (size_t)b->nq * STATS_WORDS * 4, hipMemcpyDeviceToHost));
  return SGPU_OK;
}

// (trace builds) the event times of the last traced cooperative launch of any pool lane of replica d
uint32_t coop_trace_dump(DeviceIndex* d, uint64_t* out, uint32_t cap) {
  if (!d) return 0;
  (void)hipSetDevice(d->device);
  Lane* lanes[DeviceIndex::kPool + 1];
  int nl = 0;
  lanes[nl++] = &d->main;
  for (Lane& l : d->pool) lanes[nl++] = &l;
  for (int i = 0; i < nl; ++i) {
    Lane* l = lanes[i];
    if (!l->coop || !l->coop_trace_n) continue;
    (void)hipStreamSynchronize(l->stream);
    const uint32_t n = std::min<uint32_t>(cap, l->coop_trace_n);
    if (hipMemcpy(out, l->coop + l->coop_trace_off, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
  }
  return 0;
}

// sgpu_summary_distances: one-query batch in MODE_DOTS; dots come back through out_scores.
sgpu_status summary_distances(DeviceIndex* d, const HostIndex& h, uint32_t list, const uint32_t* comps,
                              const float* vals, uint32_t nnz, float* out_dots, uint32_t* out_nb) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (list >= h.dim) return fail(SGPU_EINVAL, "list %u >= dim", list);
  const uint32_t nb = (uint32_t)(h.list_block_start[list + 1] - h.list_block_start[list]);
  *out_nb = nb;
  if (nb == 0 || nnz == 0) {
    for (uint32_t i = 0; i < nb; ++i) out_dots[i] = 0.0f;
    return SGPU_OK;
  }
  // MODE_DOTS runs stages 0-1 of the search kernel for one query, aimed at `list`
  // (KParams::target_list, carried here in query_cut), and dumps the accumulators.
  const uint64_t q_off[2] = {0, nnz};
  sgpu_batch* b = nullptr;
  sgpu_status st = batch_create(d, &d->main, h.dim, q_off, comps, vals, 1, 1, &b);
  if (st != SGPU_OK) return st;
  sgpu_search_params sp{};
  sp.k = 1;
  sp.query_cut = list;   // MODE_DOTS: carries the target list id
  sp.heap_factor = 0;
  st = batch_run(d, nullptr, b, sp, MODE_DOTS, 1, nullptr);
  if (st == SGPU_OK) {
    if (hipMemcpy(out_dots, b->out_scores, (size_t)nb * 4, hipMemcpyDeviceToHost) != hipSuccess)
      st = fail(SGPU_EDEVICE, "hipMemcpy of summary dots failed");
  }
  batch_free(b);
  return st;
}

// Knn::new (reference src/inverted_index.rs:448-500): every document is used as a query with
// k = nknn + 1, query_cut = 10, heap_factor = 0.7, first_sorted = false; itself is removed, the
// first nknn remaining results are its neighbours; lists are flattened in document order (a
// document with fewer results contributes fewer ids, exactly as the reference's flatten does).
// The N_docs searches run as batches through the same GPU kernel.
sgpu_status build_knn_on_device(DeviceIndex* d, HostIndex& h, uint32_t nknn) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (nknn == 0 || nknn + 1 > 1024) return fail(SGPU_EINVAL, "nknn must be in 1..1023");
  const uint32_t k = nknn + 1;
  const uint64_t chunk = hook_u32("SGPU_KNN_CHUNK", 32768);
  std::vector<uint32_t> out;
  out.reserve((size_t)h.n_docs * nknn);
  sgpu_search_params sp{};
  sp.k = k;
  sp.query_cut = 10;
  sp.heap_factor = 0.7f;
  sp.n_knn = 0;
  sp.first_sorted = 0;
  // make sure no stale graph is used while building
  sgpu_status st = device_index_set_knn(d, {}, 0);
  if (st != SGPU_OK) return st;
  std::vector<uint64_t> q_off;
  std::vector<uint32_t> q_comp;
  std::vector<float> q_val, sc;
  std::vector<uint64_t> ids;
  std::vector<uint32_t> n;
  for (uint64_t d0 = 0; d0 < h.n_docs; d0 += chunk) {
    const uint64_t d1 = std::min<uint64_t>(h.n_docs, d0 + chunk);
    const uint32_t nq = (uint32_t)(d1 - d0);
    const uint64_t e0 = h.fwd_offsets[d0], e1 = h.fwd_offsets[d1];
    q_off.resize(nq + 1);
    q_comp.resize(e1 - e0);
    q_val.resize(e1 - e0);
    for (uint32_t q = 0; q <= nq; ++q) q_off[q] = h.fwd_offsets[d0 + q] - e0;
    for (uint64_t i = e0; i < e1; ++i) {
      q_comp[i - e0] = h.comp(i);
      q_val[i - e0] = h.val(i);
    }
    sgpu_batch* b = nullptr;
    st = batch_create(d, &d->main, h.dim, q_off.data(), q_comp.data(), q_val.data(), nq, k, &b);
    if (st != SGPU_OK) return st;
    st = batch_run(d, nullptr, b, sp, MODE_SEARCH, 1, nullptr);
    sc.resize((size_t)nq * k);
    ids.resize((size_t)nq * k);
    n.resize(nq);
    if (st == SGPU_OK) st = batch_fetch(d, nullptr, b, k, sc.data(), ids.data(), n.data());
    batch_free(b);
    if (st != SGPU_OK) return st;
    for (uint32_t q = 0; q < nq; ++q) {
      uint32_t taken = 0;
      for (uint32_t i = 0; i < n[q] && taken < nknn; ++i) {
        const uint64_t id = ids[(size_t)q * k + i];
        if (id == d0 + q) continue;   // remove the document itself
        out.push_back((uint32_t)id);
        ++taken;
      }
    }
  }
  h.knn.swap(out);
  h.knn_dim = nknn;
  return device_index_set_knn(d, h.knn, h.knn_dim);
}

}  // namespace sgpu
