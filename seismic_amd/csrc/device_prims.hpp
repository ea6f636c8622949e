// device_prims.hpp — the small device functions the kernels beside the search kernels share (exact_device.hip, the
// candidate calls' units through score_lookup.hpp, filter.hip, build_summaries.hip, build_assign.hip): one definition each. The binary16 conversion
// is record.hpp's half_bits_to_float.
#pragma once
#include "record.hpp"

namespace sgpu {

// The monotone u32 image of an f32: all bits of a negative flipped, the sign bit of the others - f32::total_cmp order as
// an unsigned key, ascending with the float (NaN aside).
SGPU_DEV uint32_t ordered_u32(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SGPU_DEV float ordered_u32_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Inclusive prefix sum over the 64 lanes of a wavefront, by shuffles (search_lds.inc has its own DPP form).
SGPU_DEV uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t lane = __lane_id();
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Reductions over a 16-lane group (xor shuffles, strides 8, 4, 2, 1: every lane ends with the result), for the kernels in
// which a group owns a document. The f32 sum is the canonical one of a score: t[j] += t[j ^ s], each step rounded once.
SGPU_DEV float group16_sum(float v) {
  v = __fadd_rn(v, __shfl_xor(v, 8, 16));
  v = __fadd_rn(v, __shfl_xor(v, 4, 16));
  v = __fadd_rn(v, __shfl_xor(v, 2, 16));
  v = __fadd_rn(v, __shfl_xor(v, 1, 16));
  return v;
}
SGPU_DEV uint32_t group16_sum(uint32_t v) {
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) v += __shfl_xor(v, s, 16);
  return v;
}
SGPU_DEV uint32_t group16_or(uint32_t v) {
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) v |= __shfl_xor(v, s, 16);
  return v;
}
SGPU_DEV uint64_t group16_max(uint64_t v) {
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) {
    const uint64_t o = __shfl_xor(v, s, 16);
    v = o > v ? o : v;
  }
  return v;
}

// Bitonic sort of the 64-bit keys[0 .. n) in LDS, n a power of two, by a TEAM of `nt` threads of which the caller is
// thread `t`; the keys are the caller's to have written and made visible (a barrier). Every step ends with
// __syncthreads(): all threads of the workgroup must call this with the same n - teams sort their own keys side by side.
template <bool DESCENDING, typename K>
SGPU_DEV void bitonic_sort_lds(K* keys, uint32_t n, uint32_t t, uint32_t nt) {
  static_assert(sizeof(K) == 8, "64-bit keys");
  for (uint32_t size = 2; size <= n; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t p = t; p < (n >> 1); p += nt) {
        const uint32_t i = 2u * p - (p & (stride - 1u)), j = i + stride;
        const K x = keys[i], y = keys[j];
        const bool forward = (i & size) == 0u;
        if ((DESCENDING ? x < y : x > y) == forward) {
          keys[i] = y;
          keys[j] = x;
        }
      }
      __syncthreads();
    }
}

// One step of a radix select over the 256 bins of `hist` (LDS), by ONE wavefront (`lane` = the caller's lane): the bin
// where the running count from the top bin down reaches `need`. sel[0] = the bin, sel[1] = what is still needed inside
// it, sel[2] = its count; sel[3] = 0 (the callers' output cursor). The barriers before and after are the caller's.
// (need and lane by reference: exact_accumulate_kernel sits at its register limit, and with them passed by value it came
// out with 44 spilled registers instead of 42 and measured 1 - 2 % slower; profiles/shared_decoder_ab.txt.)
SGPU_DEV void radix_select_pick(const uint32_t* hist, const uint32_t& need, const uint32_t& lane, uint32_t* sel) {
  uint32_t h[4], s = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    h[i] = hist[255 - 4 * lane - i];
    s += h[i];
  }
  const uint32_t incl = wave_incl_scan(s);
  uint32_t above = incl - s;
  if (above < need && need <= incl) {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      if (above < need && need <= above + h[i]) {
        sel[0] = 255 - 4 * lane - i;
        sel[1] = need - above;
        sel[2] = h[i];
      }
      above += h[i];
    }
  }
  sel[3] = 0;
}

}  // namespace sgpu
