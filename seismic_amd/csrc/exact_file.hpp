// exact_file.hpp — the "exact file" of a replica as the launchers that read it see it (exact_device.hip builds and owns it;
// term_filter.hip reads it): the complete, unpruned inverted file of the forward index, keyed by (range of kExactRange
// documents, component), one u32 per stored component: local id in the low 16 bits, the stored value in the index's own
// encoding (f16 bits or a u8 code) in the high 16.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "hip_util.hpp"

namespace sgpu {

constexpr uint32_t kExactRangeBits = 15, kExactRange = 1u << kExactRangeBits;   // documents per range (u16 local ids)

struct ExactFile {
  int device = -1;
  uint32_t n_cu = 0;
  hipStream_t stream = nullptr;
  uint64_t n_docs = 0, dim = 0;
  uint32_t n_ranges = 0, f16 = 1;
  float val_scale = 0.0f;
  DeviceBuffer ent, off, rbase;   // the file: u32 entries, u32 offsets [range][dim + 1], u64 base per range
  uint64_t bytes = 0;
  std::mutex mu;   // one call at a time on this file (its stream and scratch): exact calls and term-filter calls take turns
  // per-call scratch, grown as calls need it: the staged queries, the chunk's candidates, the call's result rows
  DeviceBuffer q_off, q_comp, q_val, cand, out_scores, out_ids, out_n;
  uint32_t last_launches = 0;   // accumulate launches of the last call (sgpu_debug_exact_launches)
  // term_filter.hip's scratch: the staged clauses, the `within` words, the result words and the count
  DeviceBuffer tf_clauses, tf_within, tf_bits, tf_count;
  hipEvent_t tf_e0 = nullptr, tf_e1 = nullptr;   // around the term-filter kernel
  float tf_kernel_ms = 0;       // kernel time of the last term-filter call (sgpu_debug_term_filter_stats)
  double build_wall_ms = 0;     // wall time of the file's build
};

// The exact file of `replica`, built there on first use (SGPU_EDEVICE: not uploaded / no such replica; SGPU_ELIMIT: the
// file's own limits; SGPU_ENOMEM). *built (may be null) = whether this call built it.
sgpu_status exact_file_get(sgpu_index* idx, uint32_t replica, ExactFile** out, bool* built = nullptr);

}  // namespace sgpu
