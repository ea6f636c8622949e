// launch_config.cpp — launch_configure: the launch configuration as a pure function of the replica's and the batch's
// figures, the launch plan, the search parameters and the knobs (launch_config.hpp). Host code: no HIP call.
#include "launch_config.hpp"

#include <cmath>

namespace sgpu {

namespace {

inline uint64_t up(uint64_t x) { return (x + 15ull) & ~15ull; }

// The dynamic LDS of a workgroup, area by area: every area starts where the one before it ended, on a multiple of 16.
// Computed in 64 bits (qc * qn reaches 2^32 for 64K-component queries) and checked against the limit before a launch
// narrows it.
struct Areas {
  uint64_t o = 0;
  uint32_t add(uint64_t bytes) {
    const uint32_t at = (uint32_t)o;
    o += up(bytes);
    return at;
  }
};

// Which launch sizes take the cooperative variant on their own. Until r05: up to n_cu queries. With the streamed plain
// variants the picture has two windows (r06, 8.8M documents, kernel us per launch, cooperative / plain - profiles/
// r06_small_launches.txt): 144 queries 304 / 326, 176: 327 / 329, 224: 351 / 339, 256: 365 / 340 - one 1024-thread streamed
// workgroup per CU beats the helpers once most CUs own a query; 288: 420 / 453, 352: 448 / 473, 416: 481 / 512, 448: 496 / 502,
// 480: 513 / 507 - past n_cu the plain launch falls back to 512-thread workgroups and the tail help pays again until ~1.75
// queries per CU. SGPU_COOP_MAX_NQ = n keeps the old rule "up to n".
bool coop_by_size(const LaunchInput& in) {
  if (in.knobs.coop_max_nq.set) return in.nq <= in.knobs.coop_max_nq.v;
  return in.nq <= in.n_cu * 11u / 16u || (in.nq > in.n_cu && in.nq <= in.n_cu * 7u / 4u);
}

}  // namespace

sgpu_status launch_configure(const LaunchInput& in, LaunchConfig* out) {
  const Knobs& kn = in.knobs;
  const sgpu_search_params& sp = in.sp;
  const uint32_t mode = in.mode;
  if (sp.k == 0) return fail(SGPU_EINVAL, "k must be > 0 (KHeap::new asserts, reference src/utils.rs:23)");
  if (sp.k > in.k_max) return fail(SGPU_EINVAL, "k = %u exceeds the batch's k_max = %u", sp.k, in.k_max);
  if (std::isnan(sp.heap_factor)) return fail(SGPU_EINVAL, "heap_factor is NaN");
  // 512 threads x 2 workgroups per CU for throughput; when the batch has no more queries than
  // CUs, one 1024-thread workgroup per query (twice the scoring lanes) is ~20% faster
  uint32_t NT = kn.block.value_or((mode != MODE_DOTS && in.nq <= in.n_cu) ? 1024 : 512);
  if (NT != 512 && NT != 1024) return fail(SGPU_EINVAL, "SGPU_BLOCK must be 512 or 1024");
  // (1024-thread variants exist for k <= 128 and never for the counted pass: device_types.hpp, variant_built)
  const uint32_t kr = heap_variant(sp.k);
  const bool counted = mode == MODE_COUNTED || kn.visited_bitmap;
  if (NT == 1024 && (counted || kr > 2)) NT = 512;
  const uint32_t qn = launch_qn(in.max_nnz);
  const bool searching = mode != MODE_DOTS;
  // lists walked per query. query_cut == 0 walks none: the reference's k_largest_by(0) selects no
  // list and the result is empty (src/inverted_index.rs:187-190); the LDS tables keep one slot.
  const uint32_t cut = mode == MODE_DOTS ? 1u : launch_cut(sp.query_cut, in.max_nnz);
  const uint32_t qc = std::max<uint32_t>(1, cut);
  const uint32_t words = in.dim / 32 + 1;   // + the word of the padding sentinel `dim`
  const bool plan = searching && in.has_plan;
  uint32_t dots_cap = plan ? in.dots_cap : std::max<uint32_t>(1, in.target_list_nb);
  const uint32_t sort_nb = (plan && sp.first_sorted) ? in.max_nb : 0;   // blocks of the largest list walked first, when it is sorted
  const uint64_t lds_limit = std::min<uint32_t>(in.max_lds ? in.max_lds : 65536, 160 * 1024);
  const uint64_t budget = kn.lds_target;   // what a workgroup may take when two of them are to share a CU

  // ---- sizes. An area's size is written once, here; the layout below and the fitting rules both use these.
  const uint64_t sz_weights = ((uint64_t)qn + 1) * 4;
  auto sz_rt_start = [&](uint64_t g) { return up(g * qn * 8); };
  auto sz_rt_mid = [&](uint64_t g) { return up(g * qn * 2); };
  auto sz_rt_pre = [&](uint64_t g) { return up(2ull * g * (qn + 1) * 4); };   // two streams (block-id halves) per list
  auto rt_bytes = [&](uint64_t g) { return sz_rt_start(g) + sz_rt_mid(g) + sz_rt_pre(g); };
  const uint64_t sz_order = up((uint64_t)sort_nb * 2);
  const uint64_t sz_part = up(2 * (NT / 64 + 1) * 4);      // two scan scratch areas, used alternately
  const uint64_t sz_heap = up((uint64_t)kr * 64 * 8);      // the top-k between replays
  const uint64_t sz_st = up(kStateWords * 4);              // state words + candidate lists
  // query lookup table: dense u8 index (1 B per vocabulary id + the padding sentinel), {bits, rank} per 32 vocabulary
  // ids, bits + 16-bit ranks (6 B per 32 ids), or hashed {component id, weight} entries (32 KB)
  const bool dense_shape = in.comp_width == 2 && in.dim <= 65535 && in.max_nnz <= 255;
  const uint64_t dense_table = up((uint64_t)in.dim + 1);
  const uint64_t dense_bytes = std::max<uint64_t>(dense_table, kn.dense_bytes), bitmap_bytes = up((uint64_t)words * 8);
  const uint64_t split_bits = up((uint64_t)words * 4), split_bytes = split_bits + up((uint64_t)words * 2);
  const uint64_t hash_bytes = (uint64_t)kHashSlots * 8;
  // What the fitting rules for the row tables and the block dots assume follows those two areas: the areas up to the
  // lookup table as they will be laid out, the lookup table by the shape of the index alone, and the union region of a
  // round of 512 items.
  const uint64_t rest = sz_order + sz_part + sz_heap + sz_st + (dense_shape ? dense_table : up((uint64_t)words * 6)) + up(512 * 16 + NT * 12);

  // ---- layout
  LdsLayout L{};
  Areas lay;
  // the weights the scoring loop reads come FIRST (LDS byte 0 is the 0.0 slot non-matching components resolve to)
  static_assert(kQscOffset == 0, "the weights come first");
  L.q_sc = lay.add(sz_weights);   // == kQscOffset: the kernel addresses the weights as byte + constant
  // f16 documents: q_sc holds the query's values themselves; fixed-u8 documents: a second copy, scaled by val_scale
  L.q_val = in.value_type != SGPU_VAL_F16 ? lay.add(sz_weights) : L.q_sc;
  L.q_comp = lay.add((uint64_t)qn * 4);
  L.sel = lay.add((6ull * qc + 1) * 4);
  // Row tables of stage 1 (matched rows of every (list, query component) pair): for all of a query's lists when
  // that - and all their block dots - fits next to everything else at 2 workgroups per CU (the benchmark
  // configurations); otherwise the lists are walked in GROUPS of at most qg lists and the tables hold one group
  // (r03 sized them for all lists: query_cut 16 x 96 query components = 29 KB, which cost the dense lookup table
  // - the 0.95-recall operating point ran the packed lookup at 0.55 of peak). Four lists keep all eight
  // wavefronts of stage 1 busy (two per list), so groups do not go below four unless asked (SGPU_LIST_GROUP).
  uint32_t qg = qc;
  if (plan && qc > 4 && lay.o + rt_bytes(qc) + rest + (uint64_t)dots_cap * 4 > budget) qg = 4;
  qg = std::max<uint32_t>(1, std::min<uint32_t>(qg, kn.list_group.value_or(qc)));
  if (lay.o + rt_bytes(qg) > lds_limit)
    return fail(SGPU_ELIMIT, "query_cut %u x %u query components do not fit the row tables in LDS", qc, qn);
  L.rt_start = lay.add(sz_rt_start(qg));
  L.rt_mid = lay.add(sz_rt_mid(qg));
  L.rt_pre = lay.add(sz_rt_pre(qg));
  // Block dots: all of a query's lists at once when that fits next to everything else at 2 workgroups
  // per CU; otherwise the kernel walks the lists in groups and the area shrinks, down to the largest
  // single list (docs/Guidelines.md:44-70: query_cut 10 over lists of 3600 blocks is 144 KB at once).
  if (plan && (uint64_t)dots_cap * 4 > 24u * 1024u) {
    const uint64_t fit = budget > lay.o + rest ? (budget - lay.o - rest) / 4 : 0;
    dots_cap = (uint32_t)std::max<uint64_t>(in.max_list_nb, std::min<uint64_t>(dots_cap, std::max<uint64_t>(fit, 6144)));
  }
  dots_cap = std::min<uint32_t>(dots_cap, kn.dots_cap);
  if (plan) dots_cap = std::max(dots_cap, in.max_list_nb);
  L.dots_cap = dots_cap;
  L.dots = lay.add((uint64_t)dots_cap * 4);
  L.order = lay.add(sz_order);
  L.part = lay.add(sz_part);
  L.heap = lay.add(sz_heap);
  L.st = lay.add(sz_st);
  if (lay.o > lds_limit)
    return fail(SGPU_ELIMIT, "query needs %llu bytes of LDS before its lookup table (dots %u blocks) > %llu available",
                (unsigned long long)lay.o, dots_cap, (unsigned long long)lds_limit);
  const uint64_t o = lay.o;   // [lookup table | union region (sort keys, item tables or ring)] follow

  // ---- variant: cooperative, streamed, or the plain round loop - each decided here, once.
  // Cooperative (small launches and their tails; DESIGN.md "Cooperative mode"): SGPU_COOP=0 disables it, SGPU_COOP=force
  // enables it for any launch and lets owners go wide without waiting for idle workgroups (the tests: the whole protocol
  // then runs inside big batches too). It is its own kernel symbol; k > 256 has none and takes the plain variant.
  // (measured r03, 8.8M documents: 1 query 133 vs 200 us, 8: 147 vs 297, 64: 316 vs 412, 256: 431 vs 486;
  // from ~1000 queries per launch on the variant's own cost - 6 % slower rounds, idle workgroups kept
  // resident - outweighs what its tail help returns: 780 vs 742 us)
  // (its helpers want 4096 bytes of union region: the region never has fewer than NT * 12)
  const bool plain_search = !counted && mode == MODE_SEARCH;
  const bool coop_force = kn.coop_mode == 2;
  const bool coop = plain_search && kn.coop_mode != 1 && !in.coop_broken && (coop_force || coop_by_size(in)) &&
                    variant_built(NT, kr, false, true);
  // Streamed stage 2 (r06, search_stream.inc "stage 2 as a stream"): plain search launches (the cooperative variant - small
  // launches - and the counted pass keep the round loop). Its union region holds a RING of item slots, a power of two: the
  // fitting loops below step `items` down by 128 as they always did; for a streamed launch 1024 items mean a ring of 1024
  // slots (20.4 KB where the round loop's tables of 1024 items take 22.5), anything from 512 on one of 512, less 256.
  // SGPU_STREAM=0 (test hook): the round loop.
  // (its dot indices are 16 bits wide: the dots area passed the limit above, so it holds 40960 block dots at most)
  const bool streamed = plain_search && !coop && kn.stream && variant_built(NT, kr, false, false, true);

  // ---- union region and lookup table
  uint64_t sort_bytes = 0;
  if (sort_nb > 1) {
    uint64_t n2 = 1;
    while (n2 < sort_nb) n2 <<= 1;
    sort_bytes = n2 * 8;
  }
  uint32_t ring_cap = std::min<uint32_t>(1024, std::max<uint32_t>(256, kn.ring_max));
  while (ring_cap & (ring_cap - 1)) ring_cap &= ring_cap - 1;
  auto ring_of = [&](uint32_t items) { return std::min<uint32_t>(ring_cap, items >= 1024 ? 1024u : (items >= 512 ? 512u : 256u)); };
  auto uni_for = [&](uint32_t items) {
    if (streamed)   // (+ room for the item tables of a kNN refinement round of at least 128 items, which uses the same region)
      return up(std::max<uint64_t>(std::max<uint64_t>(stream_ring_bytes(ring_of(items)), 128 * 16 + NT * 12), sort_bytes));
    return up(std::max<uint64_t>((uint64_t)items * 16 + NT * 12, sort_bytes));
  };
  // the round's item tables shrink (down to 256 items) if that is what keeps 2 workgroups per CU
  const uint32_t want_items = kn.items_max.v;
  uint32_t items_max = want_items;
  const bool dense_ok = dense_shape && !kn.no_dense && searching;
  if (!kn.items_max.set) {
    if (dense_ok)   // the dense table is worth smaller rounds (down to 512 items)
      while (items_max > 512 && o + dense_bytes + uni_for(items_max) > budget) items_max -= 128;
    if (!dense_ok || o + dense_bytes + uni_for(items_max) > budget) {
      const uint64_t smallest_lookup = (in.comp_width == 4) ? split_bytes : bitmap_bytes;
      items_max = want_items;
      while (items_max > 256 && o + smallest_lookup + uni_for(items_max) > budget) items_max -= 128;
    }
  }
  // dense when it is allowed and fits at 2 workgroups per CU
  const uint64_t min_uni = uni_for(items_max);
  const bool dense = dense_ok && (o + dense_bytes + min_uni <= budget || kn.force_dense);
  // large vocabularies: bits + 16-bit ranks (6 B per 32 ids) when the packed table (8 B) would
  // cost the second workgroup per CU
  const bool split = !dense && in.comp_width == 4 && in.max_nnz <= 65535 && (o + bitmap_bytes + min_uni > budget || kn.force_split) &&
                     !kn.no_split;
  // hashed entries: ONE LDS read per document component where the dense byte table needs two
  // (profiles/r03_lds_sensitivity.md) - preferred whenever every query of the batch has a collision-free seed, the launch
  // order (which carries the seeds) is in use, and it fits at 2 workgroups per CU (the round's item tables shrink for it as
  // they do for the dense table)
  // (measured r03 on the 8.8M-document shape, u16 components: 6.46 ms per launch against the dense byte
  // table's 5.81 - a random 8-byte read costs two bank passes where the byte read costs one and the dense
  // layout's second read is mostly a broadcast of one address; fixed-u8 6.36 against 5.56. The hashed
  // entries therefore serve u32 components, where they replace a byte read PLUS an 8-byte read; the u16
  // hashed families were dropped in r05 - u16 components use the dense table or the packed words.)
  const bool hash_family = in.comp_width == 4 && in.value_type == SGPU_VAL_F16;   // (the hashed kernels: u32 components, f16 values)
  bool hashed = hash_family && plan && in.hash_ok && !kn.no_lpt && !kn.no_hash && !kn.force_split && !kn.force_dense;
  if (hashed && !kn.force_hash) {
    uint32_t im = items_max;
    if (!kn.items_max.set) {
      im = want_items;
      while (im > 512 && o + hash_bytes + uni_for(im) > budget) im -= 128;
    }
    if (o + hash_bytes + uni_for(im) <= budget) {
      items_max = im;
    } else {
      // Past the budget the hashed table is declined for occupancy's sake - unless it is the ONLY layout the launch can
      // have: a vocabulary above ~650 000 ids has no packed (8 B per 32 ids) or split (6 B) table inside the LDS limit,
      // and declining the 32 KB of hashed entries there turned a search that fits (one workgroup per CU) into SGPU_ELIMIT.
      const bool split_allowed = in.max_nnz <= 65535 && !kn.no_split;
      const uint64_t fallback_bytes = split_allowed ? split_bytes : bitmap_bytes;
      const bool fallback_fits = o + fallback_bytes + min_uni <= lds_limit;
      if (!fallback_fits && o + hash_bytes + uni_for(im) <= lds_limit) items_max = im;
      else hashed = false;
    }
  }
  const uint32_t lookup = hashed ? LK_HASH : (dense ? LK_DENSE : (split ? LK_SPLIT : LK_PACKED));
  const uint64_t lookup_bytes = !searching ? 0u : (hashed ? hash_bytes : (dense ? dense_bytes : (split ? split_bytes : bitmap_bytes)));
  L.q_bits = (uint32_t)lay.o;
  L.q_rank = (uint32_t)(lay.o + (split && !hashed ? split_bits : lookup_bytes));
  lay.o += lookup_bytes;
  L.uni = (uint32_t)std::min<uint64_t>(lay.o, 0xffffffffu);
  const uint64_t uni = uni_for(items_max);
  lay.o += uni;
  L.qc = qc;
  L.qn = qn;
  L.qg = qg;
  if (lay.o > lds_limit)
    return fail(SGPU_ELIMIT,
                "query needs %llu bytes of LDS (dots %u blocks, %u-word bitmap, sort %llu B) > %llu available; "
                "lower query_cut / use first_sorted=0 / rebuild with a smaller centroid_fraction",
                (unsigned long long)lay.o, dots_cap, words, (unsigned long long)sort_bytes, (unsigned long long)lds_limit);
  L.total = (uint32_t)lay.o;

  LaunchConfig& c = *out;
  c = LaunchConfig{};
  c.L = L;
  c.lookup = lookup;
  c.block = NT;
  c.lds_bytes = L.total;
  c.counted = counted ? 1u : 0u;
  c.streamed = streamed ? 1u : 0u;
  c.coop = coop ? (coop_force ? 2u : 1u) : 0u;
  // (a streamed launch: the ring the region was sized for; items_max is then what is left for the item tables of a kNN
  // refinement round in the same region)
  c.ring = streamed ? ring_of(items_max) : 0u;
  if (streamed) items_max = std::max<uint32_t>(128, std::min<uint32_t>(1024, (uint32_t)((uni - NT * 12) / 16) & ~127u));
  KParams& p = c.p;
  p.k = sp.k;
  p.query_cut = cut;
  p.heap_factor = sp.heap_factor;
  p.first_sorted = sp.first_sorted != 0;
  p.mode = mode == MODE_COUNTED ? (uint32_t)MODE_SEARCH : mode;
  p.n_knn = searching ? sp.n_knn : 0u;   // ignored when the index has no graph, as the reference does
  p.items_max = items_max;
  p.items_init = std::min<uint32_t>(items_max, kn.items_init.v);
  p.items_min = std::min<uint32_t>(p.items_init, kn.items_min);
  p.rblocks_max = std::min<uint32_t>(32, std::max<uint32_t>(1, kn.rblocks));   // one mask bit per block
  p.target_list = searching ? 0 : sp.query_cut;
  p.val_scale = in.val_scale;
  p.queue_base = in.staged ? in.queue_base : 0u;
  p.ring = c.ring;
  if (streamed) {
    p.items_init = std::min<uint32_t>(std::min<uint32_t>(kn.items_init.v, 1024), c.ring);
    p.items_min = std::min<uint32_t>(p.items_min, p.items_init);
  }
  if (coop) {
    const uint64_t uni_bytes = c.lds_bytes - L.uni;
    c.max_pos = std::min<uint32_t>(65535u, std::max<uint32_t>(dots_cap, 1u));
    c.max_cand = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(kn.coop_max_cand, NT), uni_bytes / 20);
    c.chunk = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(std::max<uint32_t>(kn.coop_chunk, 1u), std::min<uint32_t>(NT, 1023u)), uni_bytes / 16);
    c.chunk_min = std::min<uint32_t>(c.chunk, std::max<uint32_t>(kn.coop_chunk_min, 1u));
    c.min_items = kn.coop_min_items;
    c.first_reach = std::max<uint32_t>(1, kn.coop_first_reach);
    c.idle_min = kn.coop_idle_min.value_or(coop_force ? 0 : 8);
    // (r05: an owner goes wide once there is ONE idle workgroup per workgroup still owning a query - until r04 eight, which
    // kept the 64 owners of a 64-query launch on their own although 192 helpers were resident: 324 -> 221 us per launch,
    // 256 queries 442 -> 380 us; profiles/r05_coop_policy.txt)
    c.idle_ratio = kn.coop_idle_ratio.value_or(coop_force ? 0 : 1);
    c.poll_sleep = std::max<uint32_t>(1, kn.coop_poll);
    // How many workgroups a latency-bound launch keeps resident (r04, measured at three operating points of the 8.8M-
    // document collection, profiles/r04_coop_grid.txt): every slot of the chip is too many for one or two queries -
    // 256 helpers attach, load the query, claim from one word and have to leave again before the launch ends: a single
    // query takes 147.6 us with 256 workgroups, 129.0 with 64 - 96 and 129.6 with 48 (the 0.95 / 0.99-recall indexes:
    // 256 -> 228, 361 -> 326 us); two queries are best served by 96 - 128 (157 -> 146 us), eight by 128 - 256 (+-1 %),
    // 32 and more by all of them. Rule: 48 + 32 per query, scaled to the chip's CU count. SGPU_COOP_GRID overrides.
    const uint32_t rule = (uint32_t)(((uint64_t)48 + 32ull * in.nq) * in.n_cu / 256);
    c.coop_grid = kn.coop_grid.value_or(0xffffffffu);
    if (c.coop_grid == 0xffffffffu) c.coop_grid = std::max<uint32_t>(rule, 8);
    // latency-bound launches bootstrap the threshold with ONE local round before they go wide
    if (in.nq <= in.n_cu && !kn.items_init.set) p.items_init = std::min<uint32_t>(p.items_max, std::max<uint32_t>(1, kn.coop_items_init));
  }
  return SGPU_OK;
}

// Every slot the occupancy query allows, but: a cooperative launch that is not forced keeps coop_grid workgroups (never
// fewer than it has queries), any cooperative launch at most 512 (the open-round bitmap of its board has 512 bits), and a
// plain launch no more workgroups than queries.
uint32_t launch_grid(const LaunchConfig& c, uint32_t nq, uint32_t occupancy_grid, uint32_t* uncapped) {
  uint32_t grid = occupancy_grid;
  if (!c.coop) return std::max<uint32_t>(1, std::min<uint32_t>(grid, nq));
  if (c.coop == 1 && c.coop_grid) grid = std::max<uint32_t>(std::min<uint32_t>(grid, c.coop_grid), std::min<uint32_t>(nq, grid));
  if (uncapped) *uncapped = grid;
  return std::min<uint32_t>(grid, 512);
}

// (test hook, no device: sgpu_debug_launch_config. The knobs come from the environment, as a launch reads them.)
sgpu_status debug_launch_config(const uint32_t* w, uint32_t n_in, float heap_factor, uint32_t* out, uint32_t n_out) {
  static_assert(sizeof(LdsLayout) == 20 * 4 && sizeof(KParams) == 14 * 4, "the flat output lists their words");
  if (n_in != 23 || n_out != 58) return fail(SGPU_EINVAL, "sgpu_debug_launch_config takes 23 input words and writes 58");
  env_refresh();
  LaunchInput in;
  in.n_cu = w[0], in.max_lds = w[1], in.comp_width = w[2], in.value_type = w[3], in.dim = w[4];
  std::memcpy(&in.val_scale, &w[5], 4);
  in.coop_broken = w[6] != 0;
  in.nq = w[7], in.max_nnz = w[8], in.k_max = w[9], in.staged = w[10] != 0;
  in.has_plan = w[11] != 0, in.dots_cap = w[12], in.max_nb = w[13], in.max_list_nb = w[14], in.hash_ok = w[15] != 0;
  in.target_list_nb = w[16];
  in.sp.k = w[17], in.sp.query_cut = w[18], in.sp.heap_factor = heap_factor, in.sp.n_knn = w[19], in.sp.first_sorted = (int32_t)w[20];
  in.mode = w[21];
  in.knobs = launch_knobs();
  LaunchConfig c;
  const sgpu_status st = launch_configure(in, &c);
  if (st != SGPU_OK) return st;
  std::memcpy(out, &c.L, 80);
  std::memcpy(out + 20, &c.p, 56);
  const uint32_t tail[17] = {c.lookup, c.block, c.lds_bytes, c.counted, c.streamed, c.ring, c.coop, c.max_pos, c.max_cand, c.chunk,
                             c.chunk_min, c.min_items, c.first_reach, c.idle_min, c.idle_ratio, c.poll_sleep, c.coop_grid};
  std::memcpy(out + 34, tail, sizeof(tail));
  uint32_t uncapped = 0;
  out[51] = w[22] ? launch_grid(c, in.nq, w[22], &uncapped) : 0u;   // (an occupancy grid of 0: no grid asked for)
  out[52] = uncapped;
  const CoopBoard bd = coop_board(out[51], c.max_pos, c.max_cand);
  out[53] = (uint32_t)bd.slots, out[54] = (uint32_t)bd.pos, out[55] = (uint32_t)bd.cand, out[56] = (uint32_t)bd.trace, out[57] = (uint32_t)bd.total;
  return SGPU_OK;
}

}  // namespace sgpu
