// filter.hip — document filters: search restricted to a set A of allowed document ids (sgpu_filter_*).
//
// The search kernel reaches documents through block_post_start, post_ref and post_doc only (and, in the refine step,
// through the kNN graph). A filter's view on a replica is the replica's DevView with those arrays replaced:
//   block_post_start'  n_blocks + 1 words: the blocks' starts in the compacted postings (a block may become empty)
//   post_ref', post_doc'  the postings of allowed documents, in their original order within each block
//   knn'               (with a graph) the graph with every neighbour outside A replaced by 0xffffffff, which the
//                      kernel skips as it skips any id >= n_docs
// Records, summaries, the row directory and the block order are the replica's: the unchanged kernel searching the
// view returns exactly what unfiltered search returns on the index with the other postings deleted (DESIGN.md
// "Document filters").
//
// The view is built on the device: flag (one ballot per 64 postings, all of post_doc read once, a count per tile of
// 2048), scan of the tile counts, scatter (the flag words, then post_ref and post_doc of the kept postings), remap of the
// block starts (one flag word and one word prefix per block). Nothing of the posting arrays crosses PCIe.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <new>
#include <vector>

#include "device_prims.hpp"
#include "filter.hpp"
#include "hip_util.hpp"
#include "term_filter.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kTileWords = 32;               // flag words (64 postings each) per tile: one wavefront's share
constexpr uint32_t kTile = 64 * kTileWords;       // postings per tile
constexpr uint32_t kBS = 256;

__device__ __forceinline__ bool allowed(const uint32_t* __restrict__ bits, uint32_t doc) {
  return (bits[doc >> 5] >> (doc & 31u)) & 1u;
}

// One wavefront per tile: flags[w] = ballot of "posting 64 w + lane is kept", tile_cnt[t] = kept postings of the tile.
__global__ __launch_bounds__(kBS) void filter_flag_kernel(const uint32_t* __restrict__ post_doc, uint64_t n_postings,
                                                          const uint32_t* __restrict__ bits, uint64_t n_words,
                                                          uint64_t n_tiles, uint64_t* __restrict__ flags,
                                                          uint32_t* __restrict__ tile_cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_tiles; t += nw) {
    uint32_t cnt = 0;
    uint64_t mine = 0;   // lane w < 32 keeps flag word w of the tile: one coalesced store at the end
#pragma unroll 4
    for (uint32_t w = 0; w < kTileWords; ++w) {
      const uint64_t p = t * kTile + (uint64_t)w * 64 + lane;
      const bool keep = p < n_postings && allowed(bits, post_doc[p]);
      const uint64_t m = __ballot(keep);
      if (lane == w) mine = m;
      cnt += (uint32_t)__popcll(m);
    }
    const uint64_t wi = t * kTileWords + lane;
    if (lane < kTileWords && wi < n_words) flags[wi] = mine;
    if (lane == 0) tile_cnt[t] = cnt;
  }
}

// One workgroup: base[t] = kept postings of the tiles before t, base[n] = all of them.
__global__ __launch_bounds__(1024) void filter_scan_kernel(const uint32_t* cnt, uint64_t n, uint32_t* base) {   // (in place: base == cnt)
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint64_t b0 = 0; b0 < n; b0 += 4 * 1024) {
    uint32_t v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t j = b0 + 4 * tid + i;
      v[i] = j < n ? cnt[j] : 0u;
      s += v[i];
    }
    const uint32_t incl = wave_incl_scan(s);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t x = 0; x < w; ++x) before += wsum[x];
    before += incl - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t j = b0 + 4 * tid + i;
      if (j < n) base[j] = before;
      before += v[i];
    }
    __syncthreads();
    if (tid == 1023) carry_s = before;
    __syncthreads();
  }
  if (tid == 0) base[n] = carry_s;
}

// One wavefront per tile: the kept postings to their compacted slots; word_base[w] = kept postings before flag word w.
__global__ __launch_bounds__(kBS) void filter_scatter_kernel(const uint64_t* __restrict__ flags, uint64_t n_words, uint64_t n_tiles,
                                                             const uint32_t* __restrict__ tile_base,
                                                             const uint64_t* __restrict__ post_ref,
                                                             const uint32_t* __restrict__ post_doc,
                                                             uint64_t* __restrict__ out_ref, uint32_t* __restrict__ out_doc,
                                                             uint32_t* __restrict__ word_base) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; t < n_tiles; t += nw) {
    uint32_t base = tile_base[t];
    for (uint32_t w = 0; w < kTileWords; ++w) {
      const uint64_t wi = t * kTileWords + w;
      if (wi >= n_words) break;
      const uint64_t m = flags[wi];
      if (lane == 0) word_base[wi] = base;
      if ((m >> lane) & 1u) {
        const uint64_t p = wi * 64 + lane;
        const uint32_t pos = base + (uint32_t)__popcll(m & below);
        out_ref[pos] = post_ref[p];
        out_doc[pos] = post_doc[p];
      }
      base += (uint32_t)__popcll(m);
    }
  }
}

// block_post_start'[b] = kept postings before block_post_start[b] (b = 0 ... n_blocks).
__global__ __launch_bounds__(kBS) void filter_blocks_kernel(const uint32_t* __restrict__ bps, uint64_t n_starts,
                                                            const uint64_t* __restrict__ flags, const uint32_t* __restrict__ word_base,
                                                            uint64_t n_words, uint32_t total, uint32_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_starts; b += stride) {
    const uint32_t p = bps[b];
    const uint64_t wi = p >> 6;
    const uint32_t r = p & 63u;
    out[b] = wi < n_words ? word_base[wi] + (r ? (uint32_t)__popcll(flags[wi] & (~0ull >> (64 - r))) : 0u) : total;
  }
}

// The kNN graph with every neighbour outside A replaced by 0xffffffff.
__global__ __launch_bounds__(kBS) void filter_knn_kernel(const uint32_t* __restrict__ knn, uint64_t n, const uint32_t* __restrict__ bits,
                                                         uint32_t n_docs, uint32_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t d = knn[i];
    out[i] = d < n_docs && allowed(bits, d) ? d : 0xffffffffu;
  }
}

}  // namespace

struct FilterView {
  FilterDeviceView pub{};
  int device = -1;
  uint64_t generation = 0;
  std::vector<void*> allocs;
  uint64_t bytes = 0;
  uint64_t n_kept = 0;       // postings of the view: what the scan counted, the size post_ref' and post_doc' were allocated with
  float build_ms = 0;        // device time of the build (events around its copies and kernels)
  double build_wall_ms = 0;  // wall time of the build, allocations included
};

// The stream of a view's build and the two events around it: gone, the stream drained first, when the build returns.
struct BuildStream {
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~BuildStream() {
    if (!s) return;
    (void)hipStreamSynchronize(s);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
  }
};

static void filter_view_free(FilterView* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  for (void* p : v->allocs) (void)hipFree(p);
  delete v;
}

}  // namespace sgpu

struct sgpu_filter {
  sgpu_index* idx = nullptr;
  std::vector<uint32_t> bits;   // ceil(n_docs / 32) words; the bits past n_docs are zero
  uint64_t count = 0;
  mutable std::mutex mu;        // the views' lazy build (the views are a cache: a const filter builds them)
  mutable std::vector<sgpu::FilterView*> views;   // per replica (null until first use)
};

namespace sgpu {

sgpu_status filter_create(sgpu_index* idx, const uint32_t* doc_ids, uint64_t n, sgpu_filter** out) {
  if (!idx || !out || (n && !doc_ids)) return fail(SGPU_EINVAL, "null argument");
  *out = nullptr;
  const uint64_t n_docs = idx->host.n_docs;
  for (uint64_t i = 0; i < n; ++i)
    if (doc_ids[i] >= n_docs)
      return fail(SGPU_EINVAL, "filter: document id %u (position %llu) >= n_docs = %llu", doc_ids[i], (unsigned long long)i,
                  (unsigned long long)n_docs);
  std::vector<uint32_t> bits;
  try {
    bits.assign((size_t)std::max<uint64_t>((n_docs + 31) / 32, 1), 0u);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  for (uint64_t i = 0; i < n; ++i) bits[doc_ids[i] >> 5] |= 1u << (doc_ids[i] & 31u);
  uint64_t count = 0;
  for (uint32_t w : bits) count += (uint64_t)__builtin_popcount(w);
  return filter_from_bits(idx, std::move(bits), count, out);
}

// The one constructor: a filter of `idx` around a finished bitmap (the id list above, the term filters of term_filter.*).
sgpu_status filter_from_bits(sgpu_index* idx, std::vector<uint32_t>&& bits, uint64_t count, sgpu_filter** out) {
  sgpu_filter* f = new (std::nothrow) sgpu_filter();
  if (!f) return fail(SGPU_ENOMEM, "out of host memory");
  f->idx = idx;
  f->bits = std::move(bits);
  f->count = count;
  *out = f;
  return SGPU_OK;
}

sgpu_status filter_get_bits(const sgpu_filter* f, uint32_t* out_words, uint64_t cap_words, uint64_t* n_words) {
  if (!f) return fail(SGPU_EINVAL, "null argument");
  const uint64_t n = f->bits.size();
  if (n_words) *n_words = n;   // (set before the size check: a call with cap_words == 0 asks for the size)
  if (cap_words < n) return fail(SGPU_EINVAL, "filter bits: %llu words given, %llu needed", (unsigned long long)cap_words, (unsigned long long)n);
  if (!out_words) return fail(SGPU_EINVAL, "null argument");
  std::copy(f->bits.begin(), f->bits.end(), out_words);
  return SGPU_OK;
}

const sgpu_index* filter_index(const sgpu_filter* f) { return f->idx; }
const uint32_t* filter_host_bits(const sgpu_filter* f) { return f->bits.data(); }
uint64_t filter_count(const sgpu_filter* f) { return f ? f->count : 0; }

uint64_t filter_device_bytes(const sgpu_filter* f) {
  if (!f) return 0;
  std::lock_guard<std::mutex> lk(f->mu);
  uint64_t b = 0;
  for (const FilterView* v : f->views)
    if (v) b += v->bytes;
  return b;
}

void filter_destroy(sgpu_filter* f) {
  if (!f) return;
  for (FilterView* v : f->views) filter_view_free(v);
  delete f;
}

// (test hook) device and wall milliseconds of the build of the view on `replica`; false before it is built
bool filter_build_times(const sgpu_filter* f, uint32_t replica, double* out2) {
  std::lock_guard<std::mutex> lk(f->mu);
  if (replica >= f->views.size() || !f->views[replica]) return false;
  out2[0] = f->views[replica]->build_ms;
  out2[1] = f->views[replica]->build_wall_ms;
  return true;
}

static sgpu_status view_build(const sgpu_filter* f, const DeviceIndex* d, uint64_t generation, FilterView* v) {
  const HostIndex& h = f->idx->host;
  const auto t0 = std::chrono::steady_clock::now();
  v->device = device_index_device(d);
  v->generation = generation;
  if (hipSetDevice(v->device) != hipSuccess) return fail(SGPU_EDEVICE, "hipSetDevice(%d) failed", v->device);
  const DevView& base = device_index_view(d);
  v->pub.view = base;
  v->pub.count = f->count;
  auto dalloc = [&](void** p, uint64_t bytes, bool keep) -> sgpu_status {
    bytes = std::max<uint64_t>(bytes, 16);
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      *p = nullptr;
      return fail(SGPU_ENOMEM, "filter view: hipMalloc of %llu bytes failed", (unsigned long long)bytes);
    }
    v->allocs.push_back(*p);   // (scratch too, until the build is done: freed with the view if it fails half way)
    if (keep) v->bytes += bytes;
    return SGPU_OK;
  };
  const uint64_t n_p = h.n_postings(), n_blocks = h.n_blocks(), n_words = (n_p + 63) / 64, n_tiles = (n_p + kTile - 1) / kTile;
  const uint64_t n_bits = f->bits.size();
  sgpu_status st;
  uint32_t* bits = nullptr;
  uint64_t* flags = nullptr;
  uint32_t *tiles = nullptr, *word_base = nullptr, *bps = nullptr, *doc = nullptr, *knn = nullptr;
  uint64_t* ref = nullptr;
  if ((st = dalloc((void**)&bits, n_bits * 4, true)) != SGPU_OK || (st = dalloc((void**)&bps, (n_blocks + 1) * 4, true)) != SGPU_OK ||
      (st = dalloc((void**)&flags, n_words * 8, false)) != SGPU_OK || (st = dalloc((void**)&tiles, (n_tiles + 1) * 4, false)) != SGPU_OK ||
      (st = dalloc((void**)&word_base, n_words * 4, false)) != SGPU_OK)
    return st;
  BuildStream bs;
  if (hipStreamCreateWithFlags(&bs.s, hipStreamNonBlocking) != hipSuccess) return fail(SGPU_EDEVICE, "hipStreamCreate failed");
  HIP_TRY(hipEventCreate(&bs.e0));
  HIP_TRY(hipEventCreate(&bs.e1));
  const hipStream_t s = bs.s;
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, v->device));
  const uint32_t waves_per_wg = kBS / 64;
  auto grid_for = [&](uint64_t units, uint64_t per_wg) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((units + per_wg - 1) / per_wg, 16ull * (uint64_t)std::max(n_cu, 1)));
  };
  (void)hipGetLastError();   // (judge these launches alone)
  HIP_TRY(hipEventRecord(bs.e0, s));
  HIP_TRY(hipMemcpyAsync(bits, f->bits.data(), n_bits * 4, hipMemcpyHostToDevice, s));
  uint32_t total = 0;
  if (n_p) {
    hipLaunchKernelGGL(filter_flag_kernel, dim3(grid_for(n_tiles, waves_per_wg)), dim3(kBS), 0, s, base.post_doc, n_p, bits, n_words,
                       n_tiles, flags, tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(1024), 0, s, tiles, n_tiles, tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&total, tiles + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if ((st = dalloc((void**)&ref, (uint64_t)total * 8, true)) != SGPU_OK || (st = dalloc((void**)&doc, (uint64_t)total * 4, true)) != SGPU_OK)
    return st;
  if (n_p) {
    hipLaunchKernelGGL(filter_scatter_kernel, dim3(grid_for(n_tiles, waves_per_wg)), dim3(kBS), 0, s, flags, n_words, n_tiles,
                       tiles, base.post_ref, base.post_doc, ref, doc, word_base);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_blocks_kernel, dim3(grid_for(n_blocks + 1, kBS)), dim3(kBS), 0, s, base.block_post_start, n_blocks + 1,
                       flags, word_base, n_words, total, bps);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemsetAsync(bps, 0, (n_blocks + 1) * 4, s));
  }
  if (base.knn && base.knn_total) {
    if ((st = dalloc((void**)&knn, base.knn_total * 4, true)) != SGPU_OK) return st;
    hipLaunchKernelGGL(filter_knn_kernel, dim3(grid_for(base.knn_total, kBS)), dim3(kBS), 0, s, base.knn, base.knn_total, bits,
                       base.n_docs, knn);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(bs.e1, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&v->build_ms, bs.e0, bs.e1));
  // the scratch goes; what stays is the view's
  for (void* p : {(void*)flags, (void*)tiles, (void*)word_base}) {
    (void)hipFree(p);
    v->allocs.erase(std::find(v->allocs.begin(), v->allocs.end(), p));
  }
  v->pub.view.block_post_start = bps;
  v->pub.view.post_ref = ref;
  v->pub.view.post_doc = doc;
  v->n_kept = total;
  if (knn) v->pub.view.knn = knn;
  v->pub.bits = bits;
  v->build_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SGPU_OK;
}

// The view on `replica`, built if it is not there or stale; f->mu is held by the caller.
static sgpu_status view_locked(const sgpu_filter* f, uint32_t replica, const FilterView** out) {
  const sgpu_index* idx = f->idx;
  if (replica >= idx->replicas.size())
    return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload) / replica out of range");
  const uint64_t gen = idx->generation.load(std::memory_order_acquire);
  // views of an older generation (another upload, another graph) are dropped before anything is built
  for (FilterView*& v : f->views)
    if (v && v->generation != gen) {
      filter_view_free(v);
      v = nullptr;
    }
  try {
    if (f->views.size() < idx->replicas.size()) f->views.resize(idx->replicas.size(), nullptr);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  if (!f->views[replica]) {
    FilterView* v = new (std::nothrow) FilterView();
    if (!v) return fail(SGPU_ENOMEM, "out of host memory");
    sgpu_status st;
    try {
      st = view_build(f, idx->replicas[replica], gen, v);
    } catch (const std::bad_alloc&) {
      st = fail(SGPU_ENOMEM, "out of host memory");
    }
    if (st != SGPU_OK) {
      const std::string msg = last_error();
      filter_view_free(v);
      last_error() = msg;
      return st;
    }
    f->views[replica] = v;
  }
  *out = f->views[replica];
  return SGPU_OK;
}

sgpu_status filter_view(const sgpu_filter* f, uint32_t replica, const FilterDeviceView** out) {
  std::lock_guard<std::mutex> lk(f->mu);
  const FilterView* v = nullptr;
  const sgpu_status st = view_locked(f, replica, &v);
  if (st == SGPU_OK) *out = &v->pub;
  return st;
}

// (test hook sgpu_debug_posting_view) The posting arrays a search on `replica` walks, copied to the host: the replica's own
// (f == null) or those of f's view there, which is obtained as a search obtains it - built on first use - and read under
// the filter's mutex. sizes5 = {block starts, postings, kNN ids, bitmap words, allowed documents} (the last two 0 without
// a filter); a null buffer is skipped, one smaller than its array is an error. One blocking copy per array.
sgpu_status debug_posting_view(sgpu_index* idx, const sgpu_filter* f, uint32_t replica, uint32_t* out_bps, uint64_t cap_bps,
                               uint64_t* out_ref, uint32_t* out_doc, uint64_t cap_post, uint32_t* out_knn, uint64_t cap_knn,
                               uint32_t* out_bits, uint64_t cap_bits, uint64_t* sizes5) {
  if (replica >= idx->replicas.size())
    return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload) / replica out of range");
  std::unique_lock<std::mutex> lk;
  const DevView* view = &device_index_view(idx->replicas[replica]);
  const uint32_t* bits = nullptr;
  uint64_t n_post = idx->host.n_postings(), n_bits = 0, count = 0;
  if (f) {
    lk = std::unique_lock<std::mutex>(f->mu);
    const FilterView* v = nullptr;
    const sgpu_status st = view_locked(f, replica, &v);
    if (st != SGPU_OK) return st;
    view = &v->pub.view;
    bits = v->pub.bits;
    n_post = v->n_kept;
    n_bits = f->bits.size();
    count = v->pub.count;
  }
  const uint64_t n_starts = idx->host.n_blocks() + 1, n_knn = view->knn ? view->knn_total : 0;
  sizes5[0] = n_starts;
  sizes5[1] = n_post;
  sizes5[2] = n_knn;
  sizes5[3] = n_bits;
  sizes5[4] = count;
  if ((out_bps && cap_bps < n_starts) || ((out_ref || out_doc) && cap_post < n_post) || (out_knn && cap_knn < n_knn) ||
      (out_bits && cap_bits < n_bits))
    return fail(SGPU_EINVAL, "buffer too small");
  HIP_TRY(hipSetDevice(device_index_device(idx->replicas[replica])));
  if (out_bps) HIP_TRY(hipMemcpy(out_bps, view->block_post_start, n_starts * 4, hipMemcpyDeviceToHost));
  if (out_ref && n_post) HIP_TRY(hipMemcpy(out_ref, view->post_ref, n_post * 8, hipMemcpyDeviceToHost));
  if (out_doc && n_post) HIP_TRY(hipMemcpy(out_doc, view->post_doc, n_post * 4, hipMemcpyDeviceToHost));
  if (out_knn && n_knn) HIP_TRY(hipMemcpy(out_knn, view->knn, n_knn * 4, hipMemcpyDeviceToHost));
  if (out_bits && n_bits) HIP_TRY(hipMemcpy(out_bits, bits, n_bits * 4, hipMemcpyDeviceToHost));
  return SGPU_OK;
}

}  // namespace sgpu
