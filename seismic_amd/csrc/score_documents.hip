// score_documents.hip — scores of caller-given documents on the device (sgpu_score_documents).
//
// A score is what the search kernels return for the document (search_kernel.inc: score_class), bit for bit: the full
// query's dot product over the document's stored values in the canonical order - 16 accumulators, element e goes to
// accumulator (e / 8) % 16 in increasing e, the partials combined by t[j] += t[j ^ s], s = 8, 4, 2, 1; f32 multiply
// then add, each rounded once. Components the query does not carry resolve to the weight 0.0 and are added as +-0.0,
// which leaves an accumulator that started at +0.0 bit-identical to skipping them; padding elements of a record carry
// the value 0 and do the same.
//
// Unit of work: a TILE of at most kScoreTile candidates of ONE query (the host cuts every query's candidate list into
// tiles; the tiles of all queries of a launch go over the grid). A workgroup keeps the query's weights in LDS - a
// dense f32 table over the vocabulary where dim + 1 floats fit kScoreDenseLds bytes, else an open-addressing hash table
// {component, weight} at most half full - and rebuilds it only when its next tile belongs to another query. Every
// candidate is scored by a 16-lane group: lane l loads elements [8 l, 8 l + 8) of each 128-element round with 16-byte
// loads, kScoreDocs candidates per group in flight. The record forms are those pack_index.cpp writes:
//   raw      [npad components (u16 / u32)][npad values (binary16 / u8 codes)], npad = len rounded up to 8
//   sliced   (DotVByte) [ns x 16 B: 96 bits of first component + gaps | codes 0-3][ns x 4 B: codes 4-7], ns = npad / 8;
//            bit 15 of the ref's length field: the document keeps the raw (u16, u8) form instead
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "device_types.hpp"
#include "host_index.hpp"

namespace sgpu {

// (device_index.hip)
int device_index_device(const DeviceIndex* d);
const DevView& device_index_view(const DeviceIndex* d);

namespace {

constexpr uint32_t kScoreTile = 128;             // candidates per tile
constexpr uint32_t kScoreDocs = 2;               // candidates a 16-lane group has in flight
constexpr uint32_t kScoreDenseLds = 128u << 10;  // the dense table is used where (dim + 1) floats fit this
constexpr uint32_t kScoreChunk = 1u << 20;       // candidates per launch (SGPU_SCORE_CHUNK overrides)
constexpr uint32_t kHashEmpty = 0xffffffffu;
constexpr uint32_t kNoQuery = 0xffffffffu;
enum { SVT_F16 = 0, SVT_U8 = 1, SVT_DVB = 2 };

struct ScoreArgs {
  const uint8_t* fwd;        // DevView::fwd (the document-major records lie at its start in both forward layouts)
  const uint64_t* doc_ref;   // DevView::doc_ref
  const uint64_t* q_off;     // the call's queries, staged
  const uint32_t* q_comp;
  const float* q_val;
  const uint4* tiles;        // {query, first candidate of the tile in this launch, candidates, 0}
  const uint32_t* cand;      // the launch's candidate ids
  float* out;                // one score per candidate of the launch
  uint32_t n_tiles;
  uint32_t dim;
  uint32_t slot_bits;        // hash table: log2 of its slots
  float val_scale;
};

__device__ __forceinline__ float half_to_f32(uint32_t h) {   // exact binary16 -> binary32
  const unsigned short b = (unsigned short)h;
  _Float16 x;
  __builtin_memcpy(&x, &b, 2);
  return (float)x;
}

struct Slice {   // 8 consecutive elements of one document, as loaded
  uint4 c0, c1;  // components (u16: c0; u32: c0, c1; sliced: the 96 gap bits in c0.xyz, codes 0-3 in c0.w)
  uint4 v;       // 8 binary16 values, or 8 codes in v.x, v.y
};

template <int CW, int VT>
__device__ __forceinline__ void load_slice(Slice& s, const uint8_t* rec, uint32_t len, bool raw, uint32_t sl) {
  const uint32_t npad = (len + 7u) & ~7u;
  if (VT == SVT_DVB && !raw) {
    s.c0 = *(const uint4*)(rec + (size_t)sl * 16u);
    s.v.x = s.c0.w;
    s.v.y = *(const uint32_t*)(rec + (size_t)(npad >> 3) * 16u + (size_t)sl * 4u);
    return;
  }
  s.c0 = *(const uint4*)(rec + (size_t)sl * 8u * CW);
  if (CW == 4) s.c1 = *(const uint4*)(rec + (size_t)sl * 32u + 16u);
  const uint8_t* pv = rec + (size_t)npad * CW;
  if (VT == SVT_F16) {
    s.v = *(const uint4*)(pv + (size_t)sl * 16u);
  } else {
    const uint2 t = *(const uint2*)(pv + (size_t)sl * 8u);
    s.v.x = t.x;
    s.v.y = t.y;
  }
}

template <int CW, int VT>
__device__ __forceinline__ void slice_components(const Slice& s, bool raw, uint32_t c[8]) {
  if (VT == SVT_DVB && !raw) {
    const uint32_t w0 = s.c0.x, w1 = s.c0.y, w2 = s.c0.z;
    uint32_t run = w0 & 0xffffu;
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
  if (CW == 2) {
    c[0] = s.c0.x & 0xffffu; c[1] = s.c0.x >> 16; c[2] = s.c0.y & 0xffffu; c[3] = s.c0.y >> 16;
    c[4] = s.c0.z & 0xffffu; c[5] = s.c0.z >> 16; c[6] = s.c0.w & 0xffffu; c[7] = s.c0.w >> 16;
  } else {
    c[0] = s.c0.x; c[1] = s.c0.y; c[2] = s.c0.z; c[3] = s.c0.w;
    c[4] = s.c1.x; c[5] = s.c1.y; c[6] = s.c1.z; c[7] = s.c1.w;
  }
}

template <int VT>
__device__ __forceinline__ float slice_value(const Slice& s, int i) {
  const uint32_t v[4] = {s.v.x, s.v.y, s.v.z, s.v.w};
  if (VT == SVT_F16) return half_to_f32((v[i >> 1] >> (16 * (i & 1))) & 0xffffu);
  return (float)((v[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

// the query's weight of component c (0.0: the query does not carry it). Dense: tab[c], c <= dim. Hash: linear probing
// from the component's slot; the table is at most half full, so a probe sequence always meets an empty slot.
template <bool DENSE>
__device__ __forceinline__ float weight_of(const uint8_t* smem, uint32_t c, uint32_t slot_bits) {
  if (DENSE) return ((const float*)smem)[c];
  const uint32_t* keys = (const uint32_t*)smem;
  const float* wts = (const float*)(smem + ((size_t)4u << slot_bits));
  const uint32_t mask = (1u << slot_bits) - 1u;
  uint32_t slot = (c * 2654435761u) >> (32u - slot_bits);
  for (;;) {
    const uint32_t k = keys[slot];
    if (k == kHashEmpty) return 0.0f;
    if (k == c) return wts[slot];
    slot = (slot + 1u) & mask;
  }
}

template <int CW, int VT, bool DENSE>
__global__ __launch_bounds__(1024) void score_documents_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t ng = nt >> 4, g = tid >> 4, l = tid & 15u;
  const uint32_t slots = 1u << a.slot_bits;
  if (DENSE) {
    for (uint32_t i = tid; i <= a.dim; i += nt) ((float*)smem)[i] = 0.0f;
  } else {
    for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
  }
  uint32_t cur_q = kNoQuery;
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint4 tile = a.tiles[t];   // (workgroup-uniform)
    if (tile.x != cur_q) {
      __syncthreads();   // every group is done with the table as it is
      if (cur_q != kNoQuery) {
        if (DENSE) {
          const uint64_t p0 = a.q_off[cur_q], p1 = a.q_off[cur_q + 1];
          for (uint64_t j = p0 + tid; j < p1; j += nt) ((float*)smem)[a.q_comp[j]] = 0.0f;
        } else {
          for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
        }
        __syncthreads();
      }
      const uint64_t b0 = a.q_off[tile.x], b1 = a.q_off[tile.x + 1];
      for (uint64_t j = b0 + tid; j < b1; j += nt) {
        const uint32_t c = a.q_comp[j];
        // fixed-u8 codes: value = code * val_scale, a power of two folded into the weight (exact), as the search kernels do
        const float w = VT == SVT_F16 ? a.q_val[j] : __fmul_rn(a.q_val[j], a.val_scale);
        if (DENSE) {
          ((float*)smem)[c] = w;
        } else {
          uint32_t* keys = (uint32_t*)smem;
          float* wts = (float*)(smem + (size_t)slots * 4u);
          uint32_t slot = (c * 2654435761u) >> (32u - a.slot_bits);
          while (atomicCAS(&keys[slot], kHashEmpty, c) != kHashEmpty) slot = (slot + 1u) & (slots - 1u);
          wts[slot] = w;
        }
      }
      __syncthreads();
      cur_q = tile.x;
    }
    for (uint32_t base = 0; base < tile.z; base += ng * kScoreDocs) {
      uint32_t len[kScoreDocs], idx[kScoreDocs];
      const uint8_t* rec[kScoreDocs];
      bool raw[kScoreDocs];
      float acc[kScoreDocs];
      uint32_t max_len = 0;
#pragma unroll
      for (uint32_t u = 0; u < kScoreDocs; ++u) {
        idx[u] = base + u * ng + g;
        const uint64_t ref = idx[u] < tile.z ? a.doc_ref[a.cand[tile.y + idx[u]]] : 0ull;
        const uint32_t lf = (uint32_t)ref & 0xffffu;
        len[u] = VT == SVT_DVB ? (lf & 0x7fffu) : lf;
        raw[u] = VT == SVT_DVB && (lf & 0x8000u) != 0u;
        rec[u] = a.fwd + (size_t)(ref >> 16) * 16u;
        acc[u] = 0.0f;
        max_len = max(max_len, len[u]);
      }
      for (uint32_t e0 = l * 8u; e0 < max_len; e0 += 128u) {
        Slice s[kScoreDocs];
#pragma unroll
        for (uint32_t u = 0; u < kScoreDocs; ++u)
          if (e0 < len[u]) load_slice<CW, VT>(s[u], rec[u], len[u], raw[u], e0 >> 3);
#pragma unroll
        for (uint32_t u = 0; u < kScoreDocs; ++u)
          if (e0 < len[u]) {
            uint32_t c[8];
            slice_components<CW, VT>(s[u], raw[u], c);
            float w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = weight_of<DENSE>(smem, c[i], a.slot_bits);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[u] = __fadd_rn(acc[u], __fmul_rn(w[i], slice_value<VT>(s[u], i)));
          }
      }
#pragma unroll
      for (uint32_t u = 0; u < kScoreDocs; ++u) {
        float r = acc[u];
        r = __fadd_rn(r, __shfl_xor(r, 8, 16));
        r = __fadd_rn(r, __shfl_xor(r, 4, 16));
        r = __fadd_rn(r, __shfl_xor(r, 2, 16));
        r = __fadd_rn(r, __shfl_xor(r, 1, 16));
        if (l == 0 && idx[u] < tile.z) a.out[tile.y + idx[u]] = r;
      }
    }
  }
}

using ScoreKernel = void (*)(ScoreArgs);
ScoreKernel score_kernel(uint32_t cw, uint32_t vt, bool dense) {
  if (vt == SGPU_VAL_DOTVBYTE) return dense ? score_documents_kernel<2, SVT_DVB, true> : score_documents_kernel<2, SVT_DVB, false>;
  if (vt == SGPU_VAL_FIXEDU8) {
    if (cw == 2) return dense ? score_documents_kernel<2, SVT_U8, true> : score_documents_kernel<2, SVT_U8, false>;
    return dense ? score_documents_kernel<4, SVT_U8, true> : score_documents_kernel<4, SVT_U8, false>;
  }
  if (cw == 2) return dense ? score_documents_kernel<2, SVT_F16, true> : score_documents_kernel<2, SVT_F16, false>;
  return dense ? score_documents_kernel<4, SVT_F16, true> : score_documents_kernel<4, SVT_F16, false>;
}

}  // namespace

#define SC_TRY(expr)                                                                                          \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      return fail(SGPU_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Per replica: the score calls' stream, their recycled scratch and what the last call measured.
struct ScoreState {
  int device = -1;
  uint32_t n_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mu;   // one score call at a time on this replica
  void* scratch[6] = {};   // q_off, comps, vals, tiles, candidate ids, scores
  uint64_t scratch_bytes[6] = {};
  std::vector<uint4> tiles;     // host staging of a launch
  std::vector<uint32_t> ids;
  double last_kernel_ms = 0;    // device time of the last call's kernels, its launches and its lookup form (sgpu_debug_score_stats)
  uint32_t last_launches = 0, last_dense = 0, last_grid = 0, last_block = 0, last_lds = 0;
};

void score_state_free(ScoreState* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : s->scratch) if (p) (void)hipFree(p);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

static sgpu_status score_state_init(ScoreState* s, int device) {
  s->device = device;
  SC_TRY(hipSetDevice(device));
  int n_cu = 0;
  SC_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  s->n_cu = (uint32_t)std::max(n_cu, 1);
  SC_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  SC_TRY(hipEventCreate(&s->ev0));
  SC_TRY(hipEventCreate(&s->ev1));
  return SGPU_OK;
}

static sgpu_status score_scratch(ScoreState* s, int i, uint64_t bytes) {
  if (s->scratch_bytes[i] >= bytes && s->scratch[i]) return SGPU_OK;
  if (s->scratch[i]) {
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(s->scratch[i]);
    s->scratch[i] = nullptr;
    s->scratch_bytes[i] = 0;
  }
  bytes = std::max<uint64_t>(bytes, 16);
  if (hipMalloc(&s->scratch[i], bytes) != hipSuccess) {
    (void)hipGetLastError();
    s->scratch[i] = nullptr;
    return fail(SGPU_ENOMEM, "out of device memory scoring documents (%llu bytes)", (unsigned long long)bytes);
  }
  s->scratch_bytes[i] = bytes;
  return SGPU_OK;
}

static bool score_hooks_on() {
  const char* t = std::getenv("SGPU_TEST_HOOKS");
  return t && *t && *t != '0';
}

static sgpu_status score_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                             const float* vals, uint32_t nq, uint32_t max_nnz, const uint64_t* cand_off, const uint64_t* cand_ids,
                             float* out_scores) {
  SC_TRY(hipSetDevice(s->device));
  s->last_kernel_ms = 0;
  s->last_launches = 0;
  // the lookup form: the dense table where the vocabulary fits, else the hash table sized for the call's longest query
  // (test hook SGPU_SCORE_LOOKUP: 1 = dense where it fits, 2 = hash)
  const uint64_t dense_bytes = ((h.dim + 1) * 4 + 15) & ~15ull;
  bool dense = dense_bytes <= kScoreDenseLds;
  if (score_hooks_on()) {
    const char* v = std::getenv("SGPU_SCORE_LOOKUP");
    if (v && *v == '2') dense = false;
  }
  uint32_t slot_bits = 6;
  while ((1u << slot_bits) < 2u * max_nnz) ++slot_bits;   // (max_nnz <= kScoreMaxQueryNnz = 8192: at most 2^14 slots, 128 KiB)
  const uint32_t lds = dense ? (uint32_t)dense_bytes : (8u << slot_bits);
  const uint32_t block = lds > (40u << 10) ? 1024u : (lds > (20u << 10) ? 512u : 256u);
  ScoreKernel kern = score_kernel(h.comp_width, h.value_type, dense);
  SC_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int per_cu = 0;
  SC_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)block, lds));
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the score kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / block));

  uint64_t budget = kScoreChunk;
  if (const char* v = std::getenv("SGPU_SCORE_CHUNK"))
    if (*v) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  budget = std::min<uint64_t>(budget, 1ull << 28);
  const uint32_t tile_max = (uint32_t)std::min<uint64_t>(kScoreTile, budget);

  const uint64_t qnnz = q_off[nq];
  sgpu_status st;
  if ((st = score_scratch(s, 0, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = score_scratch(s, 1, qnnz * 4)) != SGPU_OK ||
      (st = score_scratch(s, 2, qnnz * 4)) != SGPU_OK)
    return st;
  SC_TRY(hipMemcpyAsync(s->scratch[0], q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (qnnz) {
    SC_TRY(hipMemcpyAsync(s->scratch[1], comps, qnnz * 4, hipMemcpyHostToDevice, s->stream));
    SC_TRY(hipMemcpyAsync(s->scratch[2], vals, qnnz * 4, hipMemcpyHostToDevice, s->stream));
  }
  ScoreArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = (const uint64_t*)s->scratch[0];
  a.q_comp = (const uint32_t*)s->scratch[1];
  a.q_val = (const float*)s->scratch[2];
  a.dim = (uint32_t)h.dim;
  a.slot_bits = slot_bits;
  a.val_scale = h.val_scale;
  s->last_dense = dense;
  s->last_block = block;
  s->last_lds = lds;

  // launches: consecutive tiles (a query's candidates in runs of at most tile_max) while they fit the budget
  uint32_t q = 0;
  uint64_t pos = 0;   // next candidate of the call
  const uint64_t total = cand_off[nq];
  while (pos < total) {
    s->tiles.clear();
    s->ids.clear();
    const uint64_t first = pos;
    while (pos < total && pos - first < budget) {
      while (cand_off[q + 1] <= pos) ++q;
      const uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(tile_max, cand_off[q + 1] - pos), budget - (pos - first));
      s->tiles.push_back(make_uint4(q, (uint32_t)(pos - first), n, 0u));
      pos += n;
    }
    const uint64_t n_cand = pos - first;
    s->ids.resize(n_cand);
    for (uint64_t i = 0; i < n_cand; ++i) s->ids[i] = (uint32_t)cand_ids[first + i];
    if ((st = score_scratch(s, 3, s->tiles.size() * sizeof(uint4))) != SGPU_OK || (st = score_scratch(s, 4, n_cand * 4)) != SGPU_OK ||
        (st = score_scratch(s, 5, n_cand * 4)) != SGPU_OK)
      return st;
    SC_TRY(hipMemcpyAsync(s->scratch[3], s->tiles.data(), s->tiles.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
    SC_TRY(hipMemcpyAsync(s->scratch[4], s->ids.data(), n_cand * 4, hipMemcpyHostToDevice, s->stream));
    a.tiles = (const uint4*)s->scratch[3];
    a.cand = (const uint32_t*)s->scratch[4];
    a.out = (float*)s->scratch[5];
    a.n_tiles = (uint32_t)s->tiles.size();
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n_tiles, (uint64_t)s->n_cu * (uint32_t)per_cu);
    s->last_grid = grid;
    SC_TRY(hipEventRecord(s->ev0, s->stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s->stream, a);
    SC_TRY(hipGetLastError());
    SC_TRY(hipEventRecord(s->ev1, s->stream));
    SC_TRY(hipMemcpyAsync(out_scores + first, s->scratch[5], n_cand * 4, hipMemcpyDeviceToHost, s->stream));
    SC_TRY(hipStreamSynchronize(s->stream));   // (the staging vectors and the scratch are the next launch's)
    float ms = 0.0f;
    SC_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_kernel_ms += ms;
    s->last_launches += 1;
  }
  return SGPU_OK;
}

sgpu_status score_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                   float* out_scores) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0;
  const sgpu_status vst = score_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, out_scores, &max_nnz);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(idx->score_mu);
    if (replica >= idx->replicas.size())
      return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload) / replica out of range");
    if (idx->score.size() != idx->replicas.size()) idx->score.resize(idx->replicas.size(), nullptr);
    if (!idx->score[replica]) {
      ScoreState* ns = new (std::nothrow) ScoreState();
      if (!ns) return fail(SGPU_ENOMEM, "out of host memory");
      const sgpu_status st = score_state_init(ns, device_index_device(idx->replicas[replica]));
      if (st != SGPU_OK) {
        const std::string msg = last_error();
        score_state_free(ns);
        last_error() = msg;
        return st;
      }
      idx->score[replica] = ns;
    }
    s = idx->score[replica];
  }
  if (nq == 0 || cand_off[nq] == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return score_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                     out_scores);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook: what the last score call on `replica` measured - out8 = {device ms of its kernels, launches, 1 = dense
// table / 0 = hash, grid, workgroup size, LDS bytes, 0, 0}. tools/score_probe.py)
bool score_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  std::lock_guard<std::mutex> lk(idx->score_mu);
  if (replica >= idx->score.size() || !idx->score[replica]) return false;
  ScoreState* s = idx->score[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[8] = {s->last_kernel_ms, (double)s->last_launches, (double)s->last_dense, (double)s->last_grid,
                       (double)s->last_block, (double)s->last_lds, 0.0, 0.0};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
}

}  // namespace sgpu
