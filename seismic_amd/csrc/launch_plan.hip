// launch_plan.hip — the launch plan of a query batch: which lists each query walks, the LDS need that follows, the order
// the queries are taken in; on the host (make_plan) and, for staged chunks, on the device (plan_kernel.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_index.hpp"
#include "hip_util.hpp"
#include "launch_config.hpp"

namespace sgpu {

// Which lists each query will walk (the device applies the same rule: query_cut heaviest
// components by f32::total_cmp, ties by ascending component), hence how many block dots it
// needs in LDS, and an a-priori cost (postings of those lists) to start long queries first.
sgpu_status make_plan(const DeviceIndex* d, const uint64_t* h_off, const uint32_t* h_comp, const float* h_val,
                      uint32_t nq, uint32_t query_cut, sgpu_batch_plan* out) {
  try {
    sgpu_batch_plan& pl = *out;
    pl.query_cut = query_cut;
    std::vector<uint64_t> keys(nq);
    uint32_t max_nb = 0, dots_cap = 1, max_list_nb = 1;
    {   // serial on purpose (an OpenMP team costs more to wake than this takes): ~60 ns per query for query_cut <= 16
      constexpr uint32_t kSmall = 16;
      std::vector<std::pair<int32_t, uint32_t>> kv;   // (large query_cut only)
      for (int64_t q = 0; q < (int64_t)nq; ++q) {
        const uint64_t qa = h_off[q], qe = h_off[q + 1];
        // the query_cut heaviest components by (f32::total_cmp descending, component ascending) - the order the
        // kernel's select_lists produces. Components arrive ascending, so of two equal keys the earlier one wins.
        int32_t tk[kSmall];
        uint32_t tc[kSmall];
        const uint32_t* sel = tc;
        size_t nl = 0;
        if (query_cut == 0) {
          // (no list is walked: the reference's k_largest_by(0))
        } else if (query_cut <= kSmall) {
          for (uint64_t i = qa; i < qe; ++i) {
            const int32_t key = total_key(h_val[i]);
            if (nl == query_cut && !(key > tk[nl - 1])) continue;
            size_t j = nl < query_cut ? nl++ : nl - 1;
            while (j > 0 && tk[j - 1] < key) {
              tk[j] = tk[j - 1];
              tc[j] = tc[j - 1];
              --j;
            }
            tk[j] = key;
            tc[j] = h_comp[i];
          }
        } else {
          kv.clear();
          for (uint64_t i = qa; i < qe; ++i) kv.emplace_back(total_key(h_val[i]), h_comp[i]);
          nl = std::min<size_t>(query_cut, kv.size());
          std::partial_sort(kv.begin(), kv.begin() + (long)nl, kv.end(),
                            [](const std::pair<int32_t, uint32_t>& a, const std::pair<int32_t, uint32_t>& c) {
                              if (a.first != c.first) return a.first > c.first;
                              return a.second < c.second;
                            });
        }
        uint64_t np = 0;
        uint32_t nb = 0;
        for (size_t i = 0; i < nl; ++i) {
          const uint32_t c = query_cut <= kSmall ? sel[i] : kv[i].second;
          nb += d->list_nb[c];
          np += d->list_np[c];
          max_list_nb = std::max(max_list_nb, d->list_nb[c]);
        }
        const uint32_t c0 = nl ? (query_cut <= kSmall ? sel[0] : kv[0].second) : 0xffffffffu;
        if (nl) max_nb = std::max(max_nb, d->list_nb[c0]);
        dots_cap = std::max(dots_cap, nb);
        keys[(size_t)q] = ((uint64_t)(0xffffffffu - (uint32_t)std::min<uint64_t>(np, 0xffffffffull)) << 32) | (uint32_t)q;
      }
    }
    pl.max_nb = max_nb;
    pl.dots_cap = dots_cap;
    pl.max_list_nb = max_list_nb;
    // longest expected first, ties in input order: ONE 64-bit key per query, the cost complemented in the high word and
    // the query in the low one, so a plain ascending integer sort (half the time of a sort of pairs through a
    // comparator, which was a quarter of the host side of a call). A cost saturates at 2^32 - 1 postings - four times the
    // postings of the whole 8.8M-document collection - beyond which queries simply keep their input order.
    std::sort(keys.begin(), keys.end());
    pl.order.resize(2 * (size_t)nq);
    for (uint32_t i = 0; i < nq; ++i) pl.order[i] = (uint32_t)keys[i];
    // LK_HASH seeds: the first multiplier of the family that sends the query's components to distinct slots
    // (component ids below 2^24; a query may fill at most a quarter of the table)
    // (only u32 components with f16 values have hashed kernels: configure; the seeds cost a millisecond of host time per
    // 10 000 queries and are not computed for the others)
    pl.hash_ok = d->view.dim < (1u << 24) && d->comp_width == 4 && d->value_type == SGPU_VAL_F16 && !hook_u32("SGPU_NO_HASH", 0);
    if (pl.hash_ok) {
      std::vector<uint32_t> stamp(kHashSlots, 0xffffffffu);
      uint32_t epoch = 0;
      for (uint32_t q = 0; q < nq && pl.hash_ok; ++q) {
        const uint64_t a = h_off[q], e = h_off[q + 1];
        uint32_t seed = kHashSeeds;
        if (e - a <= kHashSlots / 4)
          for (uint32_t s = 0; s < kHashSeeds && seed == kHashSeeds; ++s) {
            const uint32_t mult = hash_mult(s);
            bool clash = false;
            for (uint64_t i = a; i < e && !clash; ++i) {
              uint32_t& slot = stamp[hash_slot(h_comp[i], mult)];
              clash = slot == epoch;
              slot = epoch;
            }
            ++epoch;
            if (!clash) seed = s;
          }
        if (seed == kHashSeeds) pl.hash_ok = false;
        pl.order[(size_t)nq + q] = seed & (kHashSeeds - 1);
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory planning a query batch");
  }
  return SGPU_OK;
}

// (test hook, no device needed: the launch plan of a batch against a host index - the processing order, the block
// dots a query needs at most, the largest list walked first / at all. sgpu_debug_plan, tests/test_abi_and_host.py.
// hash_ok_out / seeds_out, where given: the plan's hash_ok and the second half of its order, one LK_HASH seed per query -
// sgpu_debug_plan_seeds, tests/test_hash_cases_cpu.py)
sgpu_status debug_plan(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                       uint32_t query_cut, uint32_t* order_out, uint32_t* out3, uint32_t* hash_ok_out, uint32_t* seeds_out) {
  DeviceIndex d;
  d.comp_width = h.comp_width;
  d.value_type = h.value_type;   // (hash_ok asks for it)
  d.view.dim = (uint32_t)h.dim;
  d.list_nb.resize(h.dim);
  d.list_np.resize(h.dim);
  for (uint64_t c = 0; c < h.dim; ++c) {
    d.list_nb[c] = (uint32_t)(h.list_block_start[c + 1] - h.list_block_start[c]);
    d.list_np[c] = (uint32_t)(h.block_post_start[h.list_block_start[c + 1]] - h.block_post_start[h.list_block_start[c]]);
  }
  sgpu_batch_plan pl;
  env_refresh();
  const sgpu_status st = make_plan(&d, q_off, comps, vals, nq, query_cut, &pl);
  if (st != SGPU_OK) return st;
  for (uint32_t i = 0; order_out && i < nq; ++i) order_out[i] = pl.order[i];
  for (uint32_t i = 0; seeds_out && i < nq; ++i) seeds_out[i] = pl.order[(size_t)nq + i];
  if (hash_ok_out) *hash_ok_out = pl.hash_ok ? 1u : 0u;
  out3[0] = pl.dots_cap;
  out3[1] = pl.max_nb;
  out3[2] = pl.max_list_nb;
  return SGPU_OK;
}

// May a launch of nq queries at this query_cut (`cut`: as staged_launch clamps it) be planned on the device? THE predicate:
// staged_launch decides with it, and search_segment (abi.cpp) asks it with the size of the chunks it is about to cut. Returns
// the block dots the LDS layout of such a launch is sized for - what earlier chunks needed (plan_dots_seen) - or 0: the host
// plans (sizes out of range, a sorted first list, the hashed lookup of u32 indexes, SGPU_DEVICE_PLAN=0, SGPU_NO_LPT, or no
// chunk has seeded the cache yet). The knobs are read through the per-call cache, which is refreshed here.
static_assert((uint32_t)kDevicePlanMaxQueries == kChunkQueriesMax, "call_cut.cpp cuts calls by kChunkQueriesMax");
uint32_t device_plan_dots(DeviceIndex* d, const sgpu_search_params& sp, uint32_t nq, uint32_t cut) {
  env_refresh();
  const bool hash_family = d->comp_width == 4 && d->value_type == SGPU_VAL_F16 && d->view.dim < (1u << 24);
  if (nq < kDevicePlanMinQueries || nq > kDevicePlanMaxQueries || cut < 1 || cut > kDevicePlanCutMax || sp.first_sorted ||
      hash_family || !env_u32("SGPU_DEVICE_PLAN", 1) || hook_u32("SGPU_NO_LPT", 0))
    return 0;
  std::lock_guard<std::mutex> lock(d->mu);
  const auto it = d->plan_dots_seen.find(cut);
  return it != d->plan_dots_seen.end() ? it->second : 0u;
}
// (SGPU_CHUNK_PLAN=device: the later chunks of a call are planned on the device as well - see staged_launch)
bool later_chunks_on_host() {
  env_refresh();
  const char* v = env_get("SGPU_CHUNK_PLAN");
  return !(v && !std::strcmp(v, "device"));
}

// (test hook: the DEVICE's launch plan of a batch - plan_kernel.hip - in the terms of debug_plan: order, out3 = {block dots
// a query needs at most, largest list walked first, largest list walked}. sgpu_debug_device_plan, tests/test_gpu_boundary.py)
sgpu_status debug_device_plan(DeviceIndex* d, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              uint32_t query_cut, uint32_t* order_out, uint32_t* out3) {
  if (!d) return fail(SGPU_EDEVICE, "index is not uploaded to a device");
  if (nq == 0 || nq > kDevicePlanMaxQueries || query_cut == 0 || query_cut > kDevicePlanCutMax)
    return fail(SGPU_EINVAL, "the device plans 1 ... %u queries at query_cut 1 ... %u", (unsigned)kDevicePlanMaxQueries, (unsigned)kDevicePlanCutMax);
  HIP_TRY(hipSetDevice(d->device));
  const uint64_t nnz = q_off[nq];
  uint32_t n2 = 2;
  while (n2 < nq) n2 <<= 1;
  std::vector<uint32_t> off32((size_t)nq + 1);
  for (uint32_t q = 0; q <= nq; ++q) off32[q] = (uint32_t)q_off[q];
  const size_t o_comp = al16((size_t)(nq + 1) * 4), o_val = o_comp + al16(nnz * 4), o_keys = o_val + al16(nnz * 4),
               o_max = o_keys + (size_t)n2 * 8, o_order = o_max + 16, total = o_order + (size_t)nq * 4;
  uint8_t* buf = nullptr;
  if (hipMalloc((void**)&buf, total) != hipSuccess) return fail(SGPU_ENOMEM, "hipMalloc of %zu bytes failed", total);
  hipError_t e = hipMemcpy(buf, off32.data(), (size_t)(nq + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && nnz) e = hipMemcpy(buf + o_comp, comps, nnz * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && nnz) e = hipMemcpy(buf + o_val, vals, nnz * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(buf + o_max, 0, 16);
  if (e == hipSuccess)
    e = launch_device_plan(d->view, (const uint32_t*)buf, (const uint32_t*)(buf + o_comp), (const float*)(buf + o_val), nq, query_cut,
                           (uint64_t*)(buf + o_keys), (uint32_t*)(buf + o_max), (uint32_t*)(buf + o_order), d->main.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(d->main.stream);
  if (e == hipSuccess) e = hipMemcpy(order_out, buf + o_order, (size_t)nq * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out3, buf + o_max, 12, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  if (e != hipSuccess) return fail(SGPU_EDEVICE, "device plan failed: %s", hipGetErrorString(e));
  return SGPU_OK;
}

sgpu_status plan_for(DeviceIndex* d, sgpu_batch* b, uint32_t query_cut, const sgpu_batch_plan** out) {
  for (const auto& pl : b->plans)
    if (pl.query_cut == query_cut) {
      *out = &pl;
      return SGPU_OK;
    }
  if (b->staged) return fail(SGPU_EINVAL, "a staged batch is planned when it is staged");
  sgpu_batch_plan pl;
  sgpu_status st = make_plan(d, b->h_off.data(), b->h_comp.data(), b->h_val.data(), b->nq, query_cut, &pl);
  if (st != SGPU_OK) return st;
  try {
    b->plans.push_back(std::move(pl));
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory planning a query batch");
  }
  *out = &b->plans.back();
  return SGPU_OK;
}

}  // namespace sgpu
