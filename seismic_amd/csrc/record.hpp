// record.hpp — a stored document record as the device reads it: the ONE place on the device that knows the layout
// pack_index.cpp writes (the one place on the host). Every kernel that scores documents from DevView::fwd - the search
// kernels (search_kernel.inc) and score_documents_kernel (score_documents.hip) - decodes through this header; how a decoded
// component finds its query weight (the lookup tables) is the kernels' own.
//
// A record holds the document's elements in slices of 8 (the last one padded); a 16-lane group reads a document one
// pass of 128 elements at a time, lane j the slice [128 s + 8 j, +8).
// VT: how the record stores values - VT_F16 (binary16, 2 bytes) or VT_U8 (fixed-u8 codes, 1 byte;
// value = code * val_scale with val_scale a power of two, folded into the weights: q_sc = q * val_scale
// is exact, and fl(q_sc * code) == fl(q * (code * val_scale)), the product the oracle computes). Both are the RAW form:
//     [npad components (u16 / u32)][npad values (binary16 / u8 codes)], npad = len rounded up to 8
// VT_DVB: the forward index of a DotVByte index (reference src/pylib/dotvbyte.rs:15-22): fixed-u8 codes as VT_U8 plus a
// COMPRESSED component stream. The reference's codec (vectorium's DotVByte, a variable-byte gap stream - not in the
// tree: parity unpinned) is lossless, so results are those of the fixed-u8 index; what is restated here is its role
// in a GPU-shaped form: per 8-element slice THREE dwords instead of four -
//     bits [0,16) the slice's first component, absolute
//     bits [16,28) [28,40) [40,52)            the gaps of elements 1, 2, 3 to their predecessors (12 bits each)
//     bits [52,63) [63,74) [74,85) [85,96)    the gaps of elements 4 .. 7 (11 bits each)
// decoded by the lane that owns the slice with nine bit-field operations and a running sum of seven additions; no
// lane needs another lane's data (the r04 first form - eight 12-bit gaps chained through the whole document - needed
// a sum of the slice, a four-step DPP scan over the document's 16 lanes and a broadcast on top: +14.5 % per launch
// against the fixed-u8 index; this form: see DESIGN.md section 5).
// Record (r05): [ns x 16 B: the slice's 12 bytes | codes of its elements 0-3][ns x 4 B: codes of elements 4-7], ns = ceil(len / 8); padding
// elements have gap 0 and code 0 (they repeat the last component with value 0: +-0.0 added, exact). A
// document with a gap that does not fit its field keeps the VT_U8 record form; bit 15 of the ref's length
// field says which (documents of a DotVByte index have < 32768 components, checked at conversion).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sgpu {

#define SGPU_DEV __device__ __forceinline__

SGPU_DEV float half_bits_to_float(uint32_t h) {   // exact binary16 -> binary32 (v_cvt_f32_f16)
  const unsigned short b = (unsigned short)h;
  _Float16 x;
  __builtin_memcpy(&x, &b, 2);
  return (float)x;
}

enum { VT_F16 = 0, VT_U8 = 1, VT_DVB = 2 };
template <int VT> struct Vt {
  static constexpr bool sliced = VT == VT_DVB;   // compressed component stream, raw fallback per document
  static constexpr bool half = VT == VT_F16;     // binary16 values (else fixed-u8 codes)
  static constexpr int raw = VT == VT_DVB ? VT_U8 : VT;   // the record form of a raw document
  static constexpr uint32_t vbytes = half ? 16u : 8u;            // value bytes per slice
};
template <int VT> struct LenMask { static constexpr uint32_t v = Vt<VT>::sliced ? 0x7fffu : 0xffffu; };
constexpr uint32_t kRawBit = 0x8000u;   // VT_DVB refs: the record is in the raw (VT_U8) form
template <typename CT, int VT>
struct DocChunk {   // 8 consecutive elements of one document, as loaded
  uint4 c0, c1, v;   // v: 8 binary16 values (16 bytes), or 8 codes in v.x, v.y; sliced (VT_DVB): the gaps in c0.x, c0.y, c0.z
};

template <int VT>
SGPU_DEV void load_values(uint4& v, const uint8_t* p) {
  if (Vt<VT>::half) {
    v = *(const uint4*)p;
  } else {
    const uint2 t = *(const uint2*)p;
    v.x = t.x;
    v.y = t.y;
  }
}

// where slice `sl` (elements [8 sl, 8 sl + 8)) of a record lies: components (or gaps) and values
template <typename CT, int VT>
SGPU_DEV void slice_ptrs(const uint8_t* rec, uint32_t len, uint32_t sl, const uint8_t*& pc, const uint8_t*& pv) {
  if (Vt<VT>::sliced) {
    // r05: [ns x 16 B: w0 w1 w2 | codes 0-3][ns x 4 B: codes 4-7] - the slice's gaps AND its first four codes in ONE
    // aligned 16-byte load, the other four codes in a dword (until r04: 12-byte slices, i.e. a 16-byte load at 4-byte
    // alignment per lane: ~4 % of a launch, profiles/r04_dvb_layouts.txt). pv is read as 8 bytes like a raw record's
    // codes (same load instruction for both record forms): the upper dword is the next slice's, ignored.
    const uint32_t ns = (len + 7u) >> 3;
    pc = rec + (size_t)sl * 16u;
    pv = rec + (size_t)ns * 16u + (size_t)sl * 4u;
  } else {
    const uint32_t npad = (len + 7u) & ~7u;
    pc = rec + (size_t)sl * 8u * sizeof(CT);
    pv = rec + (size_t)npad * sizeof(CT) + (size_t)sl * Vt<VT>::vbytes;
  }
}

template <typename CT, int VT>
SGPU_DEV void load_slice(DocChunk<CT, VT>& d, const uint8_t* pc, const uint8_t* pv) {
  d.c0 = *(const uint4*)pc;   // (VT_DVB: w0 w1 w2 | codes 0-3; v.x = codes 4-7: place_values puts them in place)
  if (!Vt<VT>::sliced && sizeof(CT) == 4) d.c1 = *(const uint4*)(pc + 16);
  load_values<VT>(d.v, pv);
}

template <typename CT, int VT>
SGPU_DEV void load_chunk(DocChunk<CT, VT>& d, const uint8_t* rec, uint32_t len, uint32_t e0) {
  const uint8_t *pc, *pv;
  slice_ptrs<CT, VT>(rec, len, e0 >> 3, pc, pv);
  load_slice<CT, VT>(d, pc, pv);
}

// The eight components of a lane's slice. Raw forms: unpacked. VT_DVB: the slice's first component and seven gaps ->
// components, plus `bias` (a dense lookup table's LDS address, so that the results are the addresses to read; 0 for
// the other layouts).
template <typename CT, int VT>
SGPU_DEV void slice_components(const DocChunk<CT, VT>& d, uint32_t c[8], uint32_t bias = 0) {
  if (Vt<VT>::sliced) {
    const uint32_t w0 = d.c0.x, w1 = d.c0.y, w2 = d.c0.z;
    uint32_t run = (w0 & 0xffffu) + bias;
    c[0] = run;
    run += (w0 >> 16) & 0xfffu;
    c[1] = run;
    run += ((w0 >> 28) | (w1 << 4)) & 0xfffu;
    c[2] = run;
    run += (w1 >> 8) & 0xfffu;
    c[3] = run;
    run += (w1 >> 20) & 0x7ffu;
    c[4] = run;
    run += ((w1 >> 31) | (w2 << 1)) & 0x7ffu;
    c[5] = run;
    run += (w2 >> 10) & 0x7ffu;
    c[6] = run;
    run += w2 >> 21;
    c[7] = run;
    return;
  }
  if (sizeof(CT) == 2) {
    c[0] = d.c0.x & 0xffffu; c[1] = d.c0.x >> 16; c[2] = d.c0.y & 0xffffu; c[3] = d.c0.y >> 16;
    c[4] = d.c0.z & 0xffffu; c[5] = d.c0.z >> 16; c[6] = d.c0.w & 0xffffu; c[7] = d.c0.w >> 16;
  } else {
    c[0] = d.c0.x; c[1] = d.c0.y; c[2] = d.c0.z; c[3] = d.c0.w;
    c[4] = d.c1.x; c[5] = d.c1.y; c[6] = d.c1.z; c[7] = d.c1.w;
  }
}

// One pass (8 elements per lane) of one document by its 16-lane group, for the loops that take a document at a time:
// `raw` = a VT_DVB index keeps this document in the VT_U8 record form (always false for the other value types).
template <typename CT, int VT>
SGPU_DEV void load_pass(DocChunk<CT, VT>& d, const uint8_t* rec, uint32_t len, bool raw, uint32_t e) {
  const uint32_t sl = (e < len ? e : 0u) >> 3;   // lanes past the end re-read the first slice
  const uint8_t *pc, *pv;
  if (Vt<VT>::sliced && raw) {
    slice_ptrs<CT, Vt<VT>::raw>(rec, len, sl, pc, pv);
    d.c0 = *(const uint4*)pc;
    load_values<Vt<VT>::raw>(d.v, pv);
  } else {
    slice_ptrs<CT, VT>(rec, len, sl, pc, pv);
    load_slice<CT, VT>(d, pc, pv);
  }
}
// ... its eight components (+ bias) where the pass was loaded with `raw` (u16 components); the others: slice_components.
// (The branch on `raw` is the caller's: with it in here the search kernels compile to other machine code.)
template <typename CT, int VT>
SGPU_DEV void raw_pass_components(const DocChunk<CT, VT>& d, uint32_t c[8], uint32_t bias = 0) {
  c[0] = (d.c0.x & 0xffffu) + bias; c[1] = (d.c0.x >> 16) + bias; c[2] = (d.c0.y & 0xffffu) + bias; c[3] = (d.c0.y >> 16) + bias;
  c[4] = (d.c0.z & 0xffffu) + bias; c[5] = (d.c0.z >> 16) + bias; c[6] = (d.c0.w & 0xffffu) + bias; c[7] = (d.c0.w >> 16) + bias;
}
// ... and its eight values put where the raw forms keep them (v; VT_DVB: the codes in v.x, v.y), in place: a packed
// slice keeps codes 0-3 behind its gaps (c0.w) and codes 4-7 in the dword v.x; a raw record's codes are v.x, v.y as loaded
template <typename CT, int VT>
SGPU_DEV void place_values(DocChunk<CT, VT>& d, bool raw) {
  if (Vt<VT>::sliced) {
    const uint32_t lo = raw ? d.v.x : d.c0.w, hi = raw ? d.v.y : d.v.x;
    d.v.x = lo;
    d.v.y = hi;
  }
}

// Value i (0 .. 7) of a slice whose values are in place (place_values), as the f32 the stored bits stand for (fixed-u8: the
// code itself - its power-of-two scale is folded into the weights). Used by score_documents_kernel only: the search
// kernels multiply straight from the stored bits (search_score.inc: mul_val).
template <int VT>
SGPU_DEV float slice_value(const uint4& val, int i) {
  const uint32_t v[4] = {val.x, val.y, val.z, val.w};
  if (Vt<VT>::half) return half_bits_to_float((v[i >> 1] >> (16 * (i & 1))) & 0xffffu);
  return (float)((v[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

}  // namespace sgpu
