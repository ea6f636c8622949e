// launch_config.hpp — everything a search launch is decided by, as a pure function: workgroup size, LDS layout, lookup
// family, item tables and ring, list groups, cooperative or streamed variant, the cooperative policy words. No HIP call,
// no allocation, no state; launch_config.cpp is host code and sgpu_debug_launch_config drives it without a device
// (tests/test_launch_config_cpu.py). DESIGN.md "Launch configuration" has the areas and the fitting rules in order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "common.hpp"
#include "device_types.hpp"

namespace sgpu {

// An environment knob whose default depends on the launch, or whose presence alone matters.
struct OptU32 {
  uint32_t v = 0;
  bool set = false;
  uint32_t value_or(uint32_t dflt) const { return set ? v : dflt; }
};

// Every SGPU_* name a launch configuration reads (knobs.cpp: launch_knobs fills it, per thread and environment).
// Runtime knobs first, test hooks - honoured only under SGPU_TEST_HOOKS=1 - after them.
struct Knobs {
  uint32_t debug = 0;              // SGPU_DEBUG
  uint32_t coop_mode = 0;          // SGPU_COOP: 0 unset (by size), 1 "0" (off), 2 "force"
  OptU32 coop_max_nq;              // SGPU_COOP_MAX_NQ: the old rule "up to n queries"
  uint32_t early_done = 1;         // SGPU_EARLY_DONE
  OptU32 block;                    // SGPU_BLOCK
  uint32_t visited_bitmap = 0;     // SGPU_VISITED_BITMAP
  OptU32 items_max;                // SGPU_ITEMS_MAX (1024): set = the fitting loops leave it alone
  OptU32 items_init;               // SGPU_ITEMS_INIT (128): set = no cooperative bootstrap round
  uint32_t items_min = 64;         // SGPU_ITEMS_MIN
  uint32_t lds_target = 160u * 1024u / 2u;   // SGPU_LDS_TARGET: the LDS budget of 2 workgroups per CU
  OptU32 list_group;               // SGPU_LIST_GROUP
  uint32_t dots_cap = 0xffffffffu; // SGPU_DOTS_CAP
  uint32_t dense_bytes = 0;        // SGPU_DENSE_BYTES
  uint32_t no_dense = 0, no_split = 0, no_hash = 0, no_lpt = 0;          // SGPU_NO_*
  uint32_t force_dense = 0, force_split = 0, force_hash = 0;             // SGPU_FORCE_*
  uint32_t stream = 1;             // SGPU_STREAM
  uint32_t ring_max = 1024;        // SGPU_RING_MAX
  uint32_t rblocks = 8;            // SGPU_RBLOCKS
  uint32_t wg_per_cu = 0;          // SGPU_WG_PER_CU (0: what the occupancy query says)
  OptU32 coop_grid;                // SGPU_COOP_GRID: unset the rule, 0 every slot, n at most n workgroups
  uint32_t coop_max_cand = 1024, coop_chunk = 128, coop_chunk_min = 4, coop_min_items = 64, coop_first_reach = 256;
  OptU32 coop_idle_min, coop_idle_ratio;   // (defaults 8 / 1, forced launches 0 / 0)
  uint32_t coop_poll = 2, coop_items_init = 128;
  uint32_t coop_reset = 0, coop_trace = 0;   // SGPU_COOP_RESET, SGPU_COOP_TRACE (device side of configure only)
};

struct LaunchInput {
  // the replica
  uint32_t n_cu = 0, max_lds = 0, comp_width = 2, value_type = SGPU_VAL_F16, dim = 0;
  float val_scale = 0.0f;
  bool coop_broken = false;
  // the batch
  uint32_t nq = 0, max_nnz = 0, k_max = 0;
  bool staged = false;
  uint32_t queue_base = 0;      // (staged batches: KParams::queue_base)
  // the launch plan of (batch, query_cut) - MODE_DOTS has none
  bool has_plan = false;
  uint32_t dots_cap = 1, max_nb = 0, max_list_nb = 1;
  bool hash_ok = false;
  uint32_t target_list_nb = 0;  // MODE_DOTS: blocks of list sp.query_cut
  sgpu_search_params sp{};
  uint32_t mode = MODE_SEARCH;
  Knobs knobs;
};

struct LaunchConfig {
  LdsLayout L;
  KParams p;
  uint32_t lookup, block, lds_bytes, counted, streamed, ring;
  uint32_t coop;        // the cooperative wish: 0 plain, 1 by size, 2 forced
  // cooperative policy words (CoopView), valid when coop != 0
  uint32_t max_pos, max_cand, chunk, chunk_min, min_items, first_reach, idle_min, idle_ratio, poll_sleep;
  uint32_t coop_grid;   // most workgroups of a cooperative launch that is not forced (0: every slot); see launch_grid
};

// Components a query's LDS tables are sized for, and the lists a search walks per query (staged_launch plans with these).
inline uint32_t launch_qn(uint32_t max_nnz) { return std::max<uint32_t>(4, (max_nnz + 3u) & ~3u); }
inline uint32_t launch_cut(uint32_t query_cut, uint32_t max_nnz) { return std::min<uint32_t>(query_cut, launch_qn(max_nnz)); }

// The configuration of one search pass, or SGPU_EINVAL / SGPU_ELIMIT with the reason in last_error().
sgpu_status launch_configure(const LaunchInput& in, LaunchConfig* out);

// Workgroups to launch, given what the occupancy query allows (n_cu x workgroups per CU). *uncapped (optional): the
// cooperative grid before the board's 512 slots cap it.
uint32_t launch_grid(const LaunchConfig& c, uint32_t nq, uint32_t occupancy_grid, uint32_t* uncapped = nullptr);

// Byte offsets of the cooperative board (CoopView) for a grid: [open 64 B | counters 64 B | slots | pos_pub | cands | trace]
struct CoopBoard {
  size_t slots, pos, cand, trace, total;
};
inline CoopBoard coop_board(uint32_t grid, uint32_t max_pos, uint32_t max_cand) {
  CoopBoard b;
  b.slots = 128;
  b.pos = b.slots + (size_t)grid * kCoopSlotWords * 8;
  b.cand = b.pos + (size_t)grid * max_pos * 8;
  b.trace = b.cand + (size_t)grid * max_cand * 16;
  b.total = b.trace + (size_t)grid * 16 * 8;
  return b;
}

// knobs.cpp: the environment behind Knobs. Names are looked at on the per-launch path, a getenv walks the whole
// environment, and a launch reads some forty of them: they are cached per thread, keyed by a fingerprint of the
// environment that env_refresh() takes once per call.
void env_refresh();
const char* env_get(const char* name);   // `name` is a string literal
uint32_t env_u32(const char* name, uint32_t dflt);
bool hooks_on();
uint32_t hook_u32(const char* name, uint32_t dflt);
const char* hook_get(const char* name);
const Knobs& launch_knobs();

// (test hook, no device: in / out are flat arrays, see sgpu_debug_launch_config in include/seismic_hip_testing.h)
sgpu_status debug_launch_config(const uint32_t* in, uint32_t n_in, float heap_factor, uint32_t* out, uint32_t n_out);

}  // namespace sgpu
