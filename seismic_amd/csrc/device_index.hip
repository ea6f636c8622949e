// device_index.hip — HBM residency of an index: upload, peer copy, free, the kNN graph, and the lanes calls run on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "device_index.hpp"
#include "hip_util.hpp"
#include "launch_config.hpp"

namespace sgpu {

static sgpu_status lane_init(Lane* l, int n_events) {
  if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(SGPU_EDEVICE, "hipStreamCreate failed");
  if (hipMalloc((void**)&l->queue, 256) != hipSuccess) return fail(SGPU_ENOMEM, "hipMalloc(queue) failed");
  if (hipMemset(l->queue, 0, 256) != hipSuccess) return fail(SGPU_EDEVICE, "hipMemset(queue) failed");   // ([32]: the lane's sticky status word)
  for (int i = 0; i < n_events; ++i) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return fail(SGPU_EDEVICE, "hipEventCreate failed");
    l->ev0.push_back(a);
    if (hipEventCreate(&b) != hipSuccess) return fail(SGPU_EDEVICE, "hipEventCreate failed");
    l->ev1.push_back(b);
  }
  return SGPU_OK;
}

static void lane_free(Lane* l) {
  if (l->stream) (void)hipStreamSynchronize(l->stream);
  if (l->scratch) batch_free(l->scratch);
  if (l->queue) (void)hipFree(l->queue);
  if (l->bitmaps) (void)hipFree(l->bitmaps);
  if (l->coop) (void)hipFree(l->coop);
  for (hipEvent_t e : l->ev0) (void)hipEventDestroy(e);
  for (hipEvent_t e : l->ev1) (void)hipEventDestroy(e);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  *l = Lane{};
}

Lane* lane_acquire(DeviceIndex* d) {
  std::unique_lock<std::mutex> lk(d->pool_mu);
  for (;;) {
    for (Lane& l : d->pool)
      if (!l.busy) {
        l.busy = true;
        return &l;
      }
    d->pool_cv.wait(lk);
  }
}

// A free lane, or null: a call that already holds one lane never WAITS for another (two callers each
// holding some lanes and waiting for more would deadlock).
Lane* lane_try_acquire(DeviceIndex* d) {
  std::lock_guard<std::mutex> lk(d->pool_mu);
  int n_free = 0;
  for (Lane& l : d->pool) n_free += !l.busy;
  if (n_free < 2) return nullptr;   // the last free lane is left to a caller that has none
  for (Lane& l : d->pool)
    if (!l.busy) {
      l.busy = true;
      return &l;
    }
  return nullptr;
}

// Is this replica serving several calls at a time? call_enter() = true when another entry-point call is in flight on it
// now or was within the last 50 ms (cut_rule, call_cut.cpp, then cuts a large call into fewer chunks: the other calls' kernels already
// hide this call's host side). The short memory matters: request threads that run in lockstep enter at the same instant,
// and the first of them would see an idle replica every time.
static inline int64_t mono_us() {
  return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
bool call_enter(DeviceIndex* d) {
  const uint32_t n = d->calls_inflight.fetch_add(1, std::memory_order_relaxed) + 1u;
  const int64_t now = mono_us();
  if (n > 1) d->concurrent_seen_us.store(now, std::memory_order_relaxed);
  return n > 1 || now - d->concurrent_seen_us.load(std::memory_order_relaxed) < 50000;
}
void call_exit(DeviceIndex* d) {
  if (d->calls_inflight.fetch_sub(1, std::memory_order_relaxed) > 1u) d->concurrent_seen_us.store(mono_us(), std::memory_order_relaxed);
}

void lane_release(DeviceIndex* d, Lane* l) {
  {
    std::lock_guard<std::mutex> lk(d->pool_mu);
    l->busy = false;
  }
  d->pool_cv.notify_one();
}

Lane* lane_main(DeviceIndex* d) { return &d->main; }
sgpu_batch** lane_scratch(Lane* l) { return &l->scratch; }

template <class T>
static sgpu_status dev_copy(DeviceIndex* d, const T* src, size_t n, const T** out) {
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  if (hipMalloc(&p, bytes) != hipSuccess) return fail(SGPU_ENOMEM, "hipMalloc of %zu bytes failed", bytes);
  d->allocs.push_back(Alloc{p, bytes, (size_t)((const char*)out - (const char*)d)});
  d->bytes += bytes;
  if (hook_get("SGPU_DEBUG_ALLOC")) std::fprintf(stderr, "sgpu alloc: field@%zu %p..%p\n", (size_t)((const char*)out - (const char*)d), p, (void*)((char*)p + bytes));
  if (n) HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *out = (const T*)p;
  return SGPU_OK;
}

void device_index_free(DeviceIndex* d) {
  if (!d) return;
  if (d->device >= 0) (void)hipSetDevice(d->device);
  lane_free(&d->main);
  for (Lane& l : d->pool) lane_free(&l);
  for (const Alloc& a : d->allocs) (void)hipFree(a.p);
  delete d;
}

uint64_t device_index_bytes(const DeviceIndex* d) { return d ? d->bytes : 0; }
int device_index_device(const DeviceIndex* d) { return d->device; }
const DevView& device_index_view(const DeviceIndex* d) { return d->view; }

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Block-major forward store: the record of every posting is copied next to the records of its
// block-mates, so that a block's documents are ONE contiguous run of HBM. One 16-lane group per
// posting, 16 bytes per lane and step (the document-major store is the source).
__global__ __launch_bounds__(256) void replicate_records_kernel(uint8_t* fwd, const uint64_t* __restrict__ doc_ref,
                                                                const uint32_t* __restrict__ post_doc,
                                                                const uint64_t* __restrict__ post_ref, uint64_t n_postings,
                                                                uint32_t bytes_per_elem, uint32_t dvb) {
  const uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const uint32_t sub = threadIdx.x & 15;
  const uint64_t n_groups = ((uint64_t)gridDim.x * blockDim.x) >> 4;
  for (uint64_t p = g; p < n_postings; p += n_groups) {
    const uint64_t dst = post_ref[p], src = doc_ref[post_doc[p]];
    uint32_t n16;   // 16-byte units of the record
    if (dvb && !(dst & 0x8000u)) {   // sliced DotVByte record: [ns x 16 B][ns x 4 B] (pack_index.cpp: record_bytes)
      const uint32_t ns = (((uint32_t)dst & 0x7fffu) + 7u) >> 3;
      n16 = (ns * 20u + 15u) >> 4;
    } else {
      const uint32_t len = (uint32_t)dst & (dvb ? 0x7fffu : 0xffffu);
      n16 = (((len + 7u) & ~7u) * bytes_per_elem + 15u) >> 4;
    }
    const uint4* s4 = (const uint4*)(fwd + (src >> 16) * 16ull);
    uint4* d4 = (uint4*)(fwd + (dst >> 16) * 16ull);
    for (uint32_t i = sub; i < n16; i += 16) d4[i] = s4[i];
  }
}

// Packs the canonical arrays into the HBM layout and copies them to `device`.
sgpu_status device_index_upload(const HostIndex& h, int device, DeviceIndex** out) {
  env_refresh();   // (SGPU_REC_LINE, SGPU_DEBUG_ALLOC: an upload runs outside any search call)
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return fail(SGPU_EDEVICE, "no HIP device available (the search path has no CPU fallback)");
  if (device < 0 || device >= n_dev) return fail(SGPU_EDEVICE, "device %d out of range (0..%d)", device, n_dev - 1);
  if (h.n_blocks() >= 0xffffffffull || h.n_postings() >= 0xffffffffull || h.n_rows() >= 0xffffffffull)
    return fail(SGPU_ELIMIT, "index too large for 32-bit device offsets (blocks / postings / summary rows)");
  HIP_TRY(hipSetDevice(device));
  DeviceIndex* d = new DeviceIndex();
  d->device = device;
  d->comp_width = h.comp_width;
  sgpu_status st = SGPU_OK;
  auto bail = [&](sgpu_status s) {
    device_index_free(d);
    return s;
  };
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(fail(SGPU_EDEVICE, "hipGetDeviceProperties failed"));
  d->n_cu = (uint32_t)prop.multiProcessorCount;
  d->max_lds = (uint32_t)prop.sharedMemPerBlock;
  if ((st = lane_init(&d->main, DeviceIndex::kMainEvents)) != SGPU_OK) return bail(st);
  for (Lane& l : d->pool)
    if ((st = lane_init(&l, 1)) != SGPU_OK) return bail(st);

  try {
    const uint32_t cw = h.comp_width, vb = h.val_bytes();
    d->value_type = h.value_type;
    d->val_scale = h.val_scale;
    // ---- document records (pack_index.cpp): [npad comps][npad values (f16, or u8 codes)], npad = len rounded up
    // to 8, the record padded to 16 bytes. A record is moved to the next 128-byte line only if it would
    // otherwise touch more lines than its size needs: at 16-byte alignment a 480-byte record straddles
    // ~4.75 lines, line-fitted 4.
    std::vector<uint64_t> rec_off16;
    std::vector<uint8_t> dvb_raw;   // DotVByte: the documents that keep the raw record form (a gap too wide for its field)
    pack_dvb_raw_flags(h, &dvb_raw);
    {
      const char* env_line = hook_get("SGPU_REC_LINE");
      pack_record_offsets(h, dvb_raw, std::max<uint64_t>(16, env_line ? std::strtoul(env_line, nullptr, 10) : 128) / 16, &rec_off16);
    }
    if (rec_off16[h.n_docs] >= (1ull << 48)) return bail(fail(SGPU_ELIMIT, "forward index exceeds 48-bit record offsets"));
    std::vector<uint8_t> fwd;
    pack_records(h, dvb_raw, rec_off16, &fwd);
    // ---- postings: (record offset / 16) << 16 | len, the reference's PackedPostingBlock
    // (src/posting_list.rs:32-60). Forward store layout:
    //   block-major (default when it fits): after the document-major records, every posting gets its
    //     own copy of its document's record, laid out block by block (a block starts on a 128-byte
    //     line, its records follow each other). A block's documents are then one contiguous run of
    //     HBM: whole lines are useful and consecutive lines share DRAM pages, where document-major
    //     records are ~4 scattered lines each with the first and last one half used. It costs
    //     n_postings / n_docs (5-6x on MS MARCO shapes: 23 GB) of the 288 GB; used up to 96 GB of copies
    //     (the 5M x 200K-vocabulary shape would take 195 GB and, not being bound by line fetches with
    //     its u32 components and packed lookup, gains nothing from them: measured 63.6% either way).
    //   document-major: one record per document, postings point into it (large indexes).
    const uint64_t doc_units = rec_off16[h.n_docs];
    std::vector<uint64_t> pref;
    uint64_t blk_units = 0;
    {
      std::vector<uint64_t> bsize;
      pack_block_sizes(h, dvb_raw, &bsize);
      blk_units = bsize[h.n_blocks()];
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      const char* env_layout = std::getenv("SGPU_FWD_LAYOUT");   // "block" | "doc"; default: block when it fits
      const uint64_t need = (doc_units + blk_units) * 16 + h.n_postings() * 24 + h.n_entries() * 8;
      bool block_major = blk_units > 0 && (doc_units + 8 + blk_units) < (1ull << 48) &&
                         need < (uint64_t)(0.6 * (double)free_b) && blk_units * 16 <= (96ull << 30);
      if (env_layout && std::strcmp(env_layout, "doc") == 0) block_major = false;
      if (env_layout && std::strcmp(env_layout, "block") == 0 && blk_units > 0) block_major = true;
      const uint64_t blk_base = (doc_units + 7) & ~7ull;
      // the store is allocated before the posting refs are laid out: if the block-major region does
      // not fit after all (memory taken by another process), the index falls back to document-major
      void* fp = nullptr;
      size_t fbytes = 0;
      for (;;) {
        const uint64_t total_units = block_major ? blk_base + blk_units : doc_units;
        fbytes = std::max<uint64_t>(total_units * 16, 16) + 16;   // (+16: a 16-byte load may start 12 bytes before the end)
        if (hipMalloc(&fp, fbytes) == hipSuccess) break;
        (void)hipGetLastError();
        if (!block_major) return bail(fail(SGPU_ENOMEM, "hipMalloc of %zu bytes failed", fbytes));
        block_major = false;
      }
      d->fwd_block_major = block_major;
      pack_post_refs(h, dvb_raw, rec_off16, bsize, block_major, blk_base, &pref);
      d->allocs.push_back(Alloc{fp, fbytes, (size_t)((const char*)&d->view.fwd - (const char*)d)});
      d->bytes += fbytes;
      d->view.fwd = (const uint8_t*)fp;
      if (hook_get("SGPU_DEBUG_ALLOC")) std::fprintf(stderr, "sgpu alloc: fwd %p..%p\n", fp, (void*)((char*)fp + fbytes));
      HIP_TRY(hipMemcpy(fp, fwd.data(), fwd.size(), hipMemcpyHostToDevice));
    }
    fwd.clear();
    fwd.shrink_to_fit();
    if ((st = dev_copy(d, pref.data(), pref.size(), &d->view.post_ref)) != SGPU_OK) return bail(st);
    {
      std::vector<uint64_t> dref;
      pack_doc_refs(h, dvb_raw, rec_off16, &dref);
      if ((st = dev_copy(d, dref.data(), dref.size(), &d->view.doc_ref)) != SGPU_OK) return bail(st);
    }
    pref.clear();
    pref.shrink_to_fit();
    if ((st = dev_copy(d, h.post_doc.data(), h.post_doc.size(), &d->view.post_doc)) != SGPU_OK) return bail(st);
    if (d->fwd_block_major && h.n_postings()) {
      (void)hipGetLastError();   // (judge this launch alone: an earlier failed call of the thread leaves its error behind)
      hipLaunchKernelGGL(replicate_records_kernel, dim3(d->n_cu * 8), dim3(256), 0, d->main.stream,
                         (uint8_t*)d->view.fwd, d->view.doc_ref, d->view.post_doc, d->view.post_ref,
                         (uint64_t)h.n_postings(), (uint32_t)(cw + vb), (uint32_t)(!dvb_raw.empty()));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(d->main.stream));
    }
    auto narrow = [](const std::vector<uint64_t>& v) {
      std::vector<uint32_t> o;
      pack_narrow(v, &o);
      return o;
    };
    {
      auto v = narrow(h.list_block_start);
      if ((st = dev_copy(d, v.data(), v.size(), &d->view.list_block_start)) != SGPU_OK) return bail(st);
      v = narrow(h.block_post_start);
      if ((st = dev_copy(d, v.data(), v.size(), &d->view.block_post_start)) != SGPU_OK) return bail(st);
    }
    if ((st = dev_copy(d, h.sum_bid.data(), h.sum_bid.size(), &d->view.sum_bid)) != SGPU_OK) return bail(st);
    {
      // split point of every summary row at half the list's block ids (rows are ascending in block
      // id, validate_desc): stage 1 gives each half of a list to its own wavefront
      std::vector<uint16_t> mid;
      pack_row_mid(h, &mid);
      d->view.list_row_start = nullptr;
      d->view.row_ptr = nullptr;
      d->view.row_comp = nullptr;
      d->view.row_mid = nullptr;
      d->view.row_dir = nullptr;
      d->view.row_dir_buckets = 0;
      if (cw == 2) {
        // u16 components: the hashed row directory IS the row index on the device - a query component's summary row
        // {first entry, entries, split point} in one trip (search_stage01.inc: build_row_table); the CSR arrays the
        // binary search of the u32 kernels walks (row_comp, row_ptr, row_mid, list_row_start: 1.7 GB for the 8.8M-document
        // index) are not uploaded at all.
        std::vector<uint32_t> dir;
        uint32_t n_buckets = 0;
        if (!pack_row_dir(h, mid, &dir, &n_buckets))
          return bail(fail(SGPU_ELIMIT, h.dim > 65535 ? "u16 components need dim <= 65535 for the device's row directory"
                                                       : "the index has too many summary rows for the device's row directory (2^31 buckets)"));
        static_assert(sizeof(d->view.row_dir) == sizeof(const uint32_t*), "pointer field");
        if ((st = dev_copy(d, dir.data(), dir.size(), (const uint32_t**)&d->view.row_dir)) != SGPU_OK) return bail(st);
        d->view.row_dir_buckets = n_buckets;
      } else {
        auto v = narrow(h.list_row_start);
        if ((st = dev_copy(d, v.data(), v.size(), &d->view.list_row_start)) != SGPU_OK) return bail(st);
        if ((st = dev_copy(d, h.row_ptr.data(), h.row_ptr.size(), &d->view.row_ptr)) != SGPU_OK) return bail(st);
        static_assert(sizeof(d->view.row_comp) == sizeof(const uint8_t*), "pointer field");
        if ((st = dev_copy(d, h.row_comp.data(), h.row_comp.size(), (const uint8_t**)&d->view.row_comp)) != SGPU_OK)
          return bail(st);
        if ((st = dev_copy(d, mid.data(), mid.size(), &d->view.row_mid)) != SGPU_OK) return bail(st);
      }
    }
    {
      // dequantised summary values: code*quant + min with the reference's two roundings
      // (src/quantized_summary.rs:102-104; this file is compiled with -ffp-contract=off)
      std::vector<float> deq;
      pack_sum_deq(h, &deq);
      if ((st = dev_copy(d, deq.data(), deq.size(), &d->view.sum_deq)) != SGPU_OK) return bail(st);
    }
    d->view.knn = nullptr;
    d->view.knn_total = 0;
    d->view.knn_dim = 0;
    if (!h.knn.empty() && h.knn_dim) {
      if ((st = dev_copy(d, h.knn.data(), h.knn.size(), &d->view.knn)) != SGPU_OK) return bail(st);
      d->view.knn_total = h.knn.size();
      d->view.knn_dim = h.knn_dim;
    }
    d->view.dim = (uint32_t)h.dim;
    d->view.n_docs = (uint32_t)h.n_docs;
    d->view.n_bitmap_words = (uint32_t)((h.n_docs + 31) / 32);
    // ---- block-count statistics for LDS sizing
    d->list_nb.resize(h.dim);
    d->list_np.resize(h.dim);
    for (uint64_t c = 0; c < h.dim; ++c) {
      d->list_nb[c] = (uint32_t)(h.list_block_start[c + 1] - h.list_block_start[c]);
      d->list_np[c] = (uint32_t)(h.block_post_start[h.list_block_start[c + 1]] - h.block_post_start[h.list_block_start[c]]);
      d->max_nb = std::max(d->max_nb, d->list_nb[c]);
    }
  } catch (const std::bad_alloc&) {
    return bail(fail(SGPU_ENOMEM, "out of host memory packing the index for upload"));
  }
  *out = d;
  return SGPU_OK;
}

// A replica of `src` on HIP device `device`: every array is copied GPU to GPU (hipMemcpyPeer goes
// over xGMI between the MI355Xs of a node; same-device "replicas" are plain device copies), nothing
// is repacked or re-sent from the host.
sgpu_status device_index_clone(const DeviceIndex* src, int device, DeviceIndex** out) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(SGPU_EDEVICE, "no HIP device available");
  if (device < 0 || device >= n_dev) return fail(SGPU_EDEVICE, "device %d out of range (0..%d)", device, n_dev - 1);
  HIP_TRY(hipSetDevice(device));
  if (device != src->device) {
    int can = 0;
    (void)hipDeviceCanAccessPeer(&can, device, src->device);
    if (can) {
      const hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    }
  }
  DeviceIndex* d = new DeviceIndex();
  d->device = device;
  d->comp_width = src->comp_width;
  d->view = src->view;
  d->n_cu = src->n_cu;
  d->max_lds = src->max_lds;
  d->list_nb = src->list_nb;
  d->list_np = src->list_np;
  d->max_nb = src->max_nb;
  d->fwd_block_major = src->fwd_block_major;
  d->value_type = src->value_type;
  d->val_scale = src->val_scale;
  auto bail = [&](sgpu_status s) {
    device_index_free(d);
    return s;
  };
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(fail(SGPU_EDEVICE, "hipGetDeviceProperties failed"));
  d->n_cu = (uint32_t)prop.multiProcessorCount;
  d->max_lds = (uint32_t)prop.sharedMemPerBlock;
  sgpu_status st;
  if ((st = lane_init(&d->main, DeviceIndex::kMainEvents)) != SGPU_OK) return bail(st);
  for (Lane& l : d->pool)
    if ((st = lane_init(&l, 1)) != SGPU_OK) return bail(st);
  // pointers of the copied view must not be freed if an allocation below fails half way
  for (const Alloc& a : src->allocs) *(const void**)((char*)d + a.field) = nullptr;
  for (const Alloc& a : src->allocs) {
    void* p = nullptr;
    if (hipMalloc(&p, a.bytes) != hipSuccess) return bail(fail(SGPU_ENOMEM, "hipMalloc of %zu bytes failed on device %d", a.bytes, device));
    d->allocs.push_back(Alloc{p, a.bytes, a.field});
    d->bytes += a.bytes;
    *(const void**)((char*)d + a.field) = p;
    const hipError_t e = hipMemcpyPeerAsync(p, device, a.p, src->device, a.bytes, d->main.stream);
    if (e != hipSuccess) return bail(fail(SGPU_EDEVICE, "hipMemcpyPeerAsync %d -> %d failed: %s", src->device, device, hipGetErrorString(e)));
  }
  if (hipStreamSynchronize(d->main.stream) != hipSuccess) return bail(fail(SGPU_EDEVICE, "peer copy failed"));
  *out = d;
  return SGPU_OK;
}

// (Re)attaches a kNN graph to a resident index.
sgpu_status device_index_set_knn(DeviceIndex* d, const std::vector<uint32_t>& knn, uint32_t knn_dim) {
  if (!d) return SGPU_OK;
  env_refresh();
  std::lock_guard<std::mutex> lock(d->mu);
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipDeviceSynchronize());
  if (d->view.knn) {   // drop the previous graph's device copy
    auto it = std::find_if(d->allocs.begin(), d->allocs.end(), [&](const Alloc& a) { return a.p == (void*)d->view.knn; });
    if (it != d->allocs.end()) d->allocs.erase(it);
    (void)hipFree((void*)d->view.knn);
    d->bytes -= std::min<uint64_t>(d->bytes, d->view.knn_total * 4);
  }
  d->view.knn = nullptr;
  d->view.knn_total = 0;
  d->view.knn_dim = 0;
  if (knn.empty() || !knn_dim) return SGPU_OK;
  sgpu_status st = dev_copy(d, knn.data(), knn.size(), &d->view.knn);
  if (st != SGPU_OK) return st;
  d->view.knn_total = knn.size();
  d->view.knn_dim = knn_dim;
  return SGPU_OK;
}

}  // namespace sgpu
