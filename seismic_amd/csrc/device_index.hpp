// device_index.hpp — private to the translation units that launch searches on a resident index (device_index.hip,
// launch_plan.hip, batch.hip, staged.hip): the structs they share and what they call of each other.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "device_calls.hpp"   // what these files export to the host side
#include "device_types.hpp"
#include "host_index.hpp"

namespace sgpu {

// One stream's worth of launch state. The device-resident batch API (sgpu_batch_*) runs on the
// index's `main` lane; sgpu_search / sgpu_batch_search borrow a lane from a small pool, so calls
// from several host threads on one index overlap (copies and kernels of different lanes run
// concurrently on the device) - the reference's `search(&self)` is re-entrant, S: Sync
// (src/index_traits.rs:106-113).
struct Lane {
  hipStream_t stream = nullptr;
  uint32_t* queue = nullptr;       // the launch's work counter (queries are pulled from it)
  // latency-bound calls (direct-in): a second counter (queue + 16) that is never reset - the host knows its value
  uint32_t queue_pos = 0;          //   ... after everything enqueued so far
  bool queue_dirty = true;         //   ... unless a launch failed (or none ran yet): zero it first
  uint32_t done_seq = 0;           // BatchView::done_seq of the lane's last early-done launch
  sgpu_batch* scratch = nullptr;   // pool lanes: the recycled device batch (no allocation per call)
  uint32_t* bitmaps = nullptr;     // visited bitmaps of the counted pass, one per resident workgroup
  uint32_t bitmaps_slots = 0;
  uint8_t* coop = nullptr;         // board of the cooperative kernel variant (CoopView), all zero between launches
  size_t coop_bytes = 0, coop_trace_off = 0;
  uint32_t coop_trace_n = 0;
  bool coop_last = false;          // the lane's last launch was a cooperative one (its board's error word is then checked)
  std::vector<hipEvent_t> ev0, ev1;   // timing of enqueued launches
  int ev_pending = 0;
  double sum_ms = 0;
  uint32_t n_timed = 0;
  sgpu_launch_stats last{};
  // (test hook sgpu_debug_lane_variant) the kernel variant of the lane's last search launch (MODE_SEARCH / MODE_COUNTED,
  // not a dots launch): {lookup (LK_*), streamed, cooperative 0 / 1 / 2 forced, counted}. configure leaves what it chose in
  // variant_next; the launcher copies it to variant once launch_search has succeeded (variant_commit). variant_set: one has
  uint32_t variant[4] = {0, 0, 0, 0}, variant_next[4] = {0, 0, 0, 0};
  bool variant_set = false;
  void variant_commit() {
    for (int i = 0; i < 4; ++i) variant[i] = variant_next[i];
    variant_set = true;
  }
  bool busy = false;
};

struct Alloc {
  void* p;
  size_t bytes;
  size_t field;   // byte offset (inside DeviceIndex) of the view pointer that refers to it
};

struct DeviceIndex {
  int device = -1;
  DevView view{};
  uint32_t comp_width = 2;
  std::vector<Alloc> allocs;
  uint64_t bytes = 0;
  uint32_t n_cu = 0;
  uint32_t max_lds = 0;
  std::vector<uint32_t> list_nb, list_np;   // blocks / postings per posting list (host copy)
  uint32_t max_nb = 0;
  uint32_t value_type = SGPU_VAL_F16;   // how the records store document values
  float val_scale = 0.0f;
  bool fwd_block_major = false;   // forward store holds a copy of every posting's record, block by block
  bool coop_broken = false;       // a cooperative launch reported a protocol error: the variant stays off for this replica
  static constexpr int kMainEvents = 64, kPool = 8;   // two concurrent calls of four chunks each
  Lane main;
  Lane pool[kPool];
  std::unordered_map<uint64_t, int> occupancy;   // kernel variant + LDS size -> workgroups per CU
  // Device-side launch plans (plan_kernel.hip): per query_cut, the largest number of block dots a query of an EARLIER chunk
  // needed (all its lists) - what the LDS layout of the next chunk is sized for; a query that needs more walks its lists in
  // groups. Seeded by the first chunk's host plan, raised by what every device plan reports back with its rows. (mu)
  std::unordered_map<uint32_t, uint32_t> plan_dots_seen;
  std::mutex mu;        // main lane, occupancy cache
  std::atomic<uint32_t> calls_inflight{0};               // entry-point calls on this replica right now (call_enter / call_exit)
  std::atomic<int64_t> concurrent_seen_us{-((int64_t)1 << 60)};   // when two of them were last seen together
  std::mutex pool_mu;   // pool lane hand-out
  std::condition_variable pool_cv;
};
}  // namespace sgpu

struct sgpu_batch_plan {   // per (batch, query_cut): LDS need and processing order (host side)
  uint32_t query_cut = 0;
  uint32_t dots_cap = 1;    // max over queries of the blocks of the lists it walks
  uint32_t max_nb = 0;      // largest single list walked first (sort buffer sizing)
  uint32_t max_list_nb = 1; // largest single list walked at all (smallest possible dots area)
  std::vector<uint32_t> order;   // queries, longest expected first; followed (second half) by every query's
                                 // LK_HASH seed: the hash multiplier under which its components do not collide
  bool hash_ok = true;           // every query of the batch has such a seed
};

// The arena of a staged batch, byte offsets:
//   [work counter 16 B | fixed status 16 B | q_off | q_comp | q_val | order | status 16 B]  ->  [out_n | out_scores | out_ids]
// (the trailing status word goes down zeroed with the input and comes back with the rows in one D2H copy; a launch that
// writes its rows straight into the pinned host arena uses the FIXED status / done words instead: their address does not
// move with nq and nnz, so a launch that is still winding down when the lane's next call stages its input - early done -
// can only ever touch those two words, never the next call's queries)
struct sgpu_staged_arena {
  size_t fix = 16, off = 32, comp = 0, val = 0, order = 0, status = 0, in_bytes = 0;   // the input region: one H2D
  size_t out_n = 0, out_scores = 0, out_ids = 0, total = 0;                             // the rows: one D2H from `status` on
  sgpu_staged_arena() = default;
  sgpu_staged_arena(size_t nq, size_t nnz, size_t k) {
    using sgpu::al16;
    comp = off + al16((nq + 1) * 4);
    val = comp + al16(nnz * 4);
    order = val + al16(nnz * 4);
    status = order + al16(nq * 8);   // [order | hash seeds]
    in_bytes = status + 16;
    out_n = in_bytes;
    out_scores = out_n + al16(nq * 4);
    out_ids = out_scores + al16(nq * k * 4);
    total = out_ids + al16(nq * k * 8);
  }
};

struct sgpu_batch {
  std::vector<uint64_t> h_off;
  std::vector<uint32_t> h_off32;   // what the device holds (the copies below read the batch's own arrays,
                                   // which live as long as the batch: nothing depends on when a copy from
                                   // pageable memory lets go of its source)
  std::vector<uint32_t> h_comp;
  std::vector<float> h_val;
  std::vector<sgpu_batch_plan> plans;
  int device = -1;
  const sgpu::DeviceIndex* owner = nullptr;   // the replica the batch was created on
  uint32_t nq = 0, k_max = 0, max_nnz = 0;
  uint64_t cap_nq = 0, cap_nnz = 0, cap_slab = 0;   // allocated capacities (a scratch batch is reused)
  uint32_t* q_off = nullptr;
  uint32_t* q_comp = nullptr;
  float* q_val = nullptr;
  uint32_t* q_order = nullptr;     // cap_nq: the processing order of the plan named by order_cut
  uint32_t* h_order = nullptr;     // its pinned host staging copy (the H2D is then truly asynchronous)
  uint32_t order_cut = 0xffffffffu;
  float* out_scores = nullptr;
  uint64_t* out_ids = nullptr;
  uint32_t* out_n = nullptr;
  uint32_t* out_stats = nullptr;   // nq x STATS_WORDS work counters of the last pass
  uint32_t* status = nullptr;      // staged batches: the launch status word (BatchView::status) as the kernel addresses it
  size_t status_off = 0;           //   ... and where it lies in the arena (the last 16 bytes of the input region)
  // Staged batches (the recycled batch of a pool lane, behind sgpu_search / sgpu_batch_search): every
  // device array above is a slice of ONE device arena mirrored by ONE pinned host buffer, so a call is
  // one H2D (work counter, queries, launch order), the kernel, one D2H (counts, scores, ids).
  bool staged = false;
  uint8_t* arena_dev = nullptr;
  uint8_t* arena_host = nullptr;
  uint8_t* arena_host_dev = nullptr;   // the pinned host arena as the device sees it (small calls write their rows straight into it)
  bool direct_out = false;
  uint32_t done_seq = 0;               // direct-out calls: the value the launch's last query stores into the arena's done word (0: none)
  bool direct_in = false;              // the kernel reads the queries from the pinned host arena (no H2D copy to enqueue)
  uint32_t queue_base = 0;             // KParams::queue_base of the next launch
  size_t arena_cap = 0;
  sgpu_staged_arena lay;               // where the chunk's arrays lie in the arena
  uint32_t* queue_dev = nullptr;
  uint32_t device_plan_cut = 0xffffffffu;   // the chunk's launch plan was computed on the device for this query_cut (its
                                            //   maxima come back in words 1 - 3 of the status block); 0xffffffff: host plan
  bool followed = false;                    // another chunk of the call comes after this one, or other calls are in flight
  bool plan_identity = false;               // a device-planned chunk that takes its queries in input order (staged_launch)
  uint32_t q_base = 0;                      // the chunk's first query in the caller's batch
};
namespace sgpu {

// launch_plan.hip (these touch nothing the lanes share)
sgpu_status make_plan(const DeviceIndex* d, const uint64_t* h_off, const uint32_t* h_comp, const float* h_val, uint32_t nq,
                      uint32_t query_cut, sgpu_batch_plan* out);
sgpu_status plan_for(DeviceIndex* d, sgpu_batch* b, uint32_t query_cut, const sgpu_batch_plan** out);
bool later_chunks_on_host();
// batch.hip
// Chooses block size, LDS layout and grid for one search pass and readies the lane for it (caller holds d->mu).
// (ov: the view to search instead of the replica's own - a filter's, filter.hip; null: the replica's)
sgpu_status configure(DeviceIndex* d, Lane* lane, sgpu_batch* b, const sgpu_search_params& sp, uint32_t mode, LaunchArgs* a,
                      const DevView* ov = nullptr);
sgpu_status coop_report(DeviceIndex* d, Lane* lane, uint32_t code);

}  // namespace sgpu
