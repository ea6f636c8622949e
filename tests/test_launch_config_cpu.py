"""The launch configuration (seismic_amd/csrc/launch_config.cpp) driven without a device through sgpu_debug_launch_config.
What is asserted follows from the kernels' contract - what search_kernel.inc reads from each LDS area, which variants the
library instantiates (device_types.hpp: variant_built), which lookup families each index type has (batch.hip: run_any), how
large the cooperative board's fields are - restated here in Python, never from the function's own output. Every edge is
an input row. A handful of deliberately WRONG readings of the contract must each fail on a named row: the rows can see that
class of bug."""
import pytest

from seismic_amd import _native
from seismic_amd._native import SeismicHipError, debug_launch_config

EINVAL, ELIMIT = 1, 5
F16, FIXEDU8, DOTVBYTE = 0, 1, 2
PACKED, DENSE, SPLIT, HASH = 0, 1, 2, 3
SEARCH, DOTS, COUNTED = 0, 1, 2
N_CU, MAX_LDS, BUDGET = 256, 160 * 1024, 80 * 1024
HOOKS = ("SGPU_FORCE_DENSE SGPU_FORCE_SPLIT SGPU_FORCE_HASH SGPU_NO_DENSE SGPU_NO_SPLIT SGPU_NO_HASH SGPU_NO_LPT SGPU_ITEMS_MAX "
         "SGPU_ITEMS_INIT SGPU_ITEMS_MIN SGPU_RING_MAX SGPU_DOTS_CAP SGPU_LDS_TARGET SGPU_BLOCK SGPU_COOP SGPU_STREAM "
         "SGPU_LIST_GROUP SGPU_COOP_MAX_NQ SGPU_COOP_GRID SGPU_VISITED_BITMAP SGPU_DENSE_BYTES SGPU_COOP_CHUNK "
         "SGPU_COOP_CHUNK_MIN SGPU_COOP_MAX_CAND SGPU_COOP_ITEMS_INIT SGPU_RBLOCKS SGPU_WG_PER_CU").split()


def up(x):
    return (x + 15) & ~15


def heap_variant(k):
    return 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16


def variant_built(block, kr, counted, coop, streamed):     # device_types.hpp
    if block not in (512, 1024) or (streamed and (counted or coop)):
        return False
    if counted:
        return block == 512
    if block == 1024:
        return kr <= 2
    return kr <= 4 if coop else True


def ring_bytes(ring):                                       # device_types.hpp: stream_ring_bytes, kStreamFeedPos = 192
    return ring * 18 + ring // 16 + 192 * 10


def configure(monkeypatch, env=None, heap_factor=1.0, **facts):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, v in (env or {}).items():
        monkeypatch.setenv(name, str(v))
    inp = dict(_native.LAUNCH_CONFIG_IN, **facts)
    return inp, debug_launch_config(heap_factor, **facts)


def violations(inp, out, env=None, reading=None):
    """Every way `out` breaks the contract for the launch `inp` under the hooks `env`. reading: one of the wrong readings of
    the contract (the tests at the end of the file)."""
    env = env or {}
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)

    o = out
    NT, kr, k = o["block"], heap_variant(inp["k"]), inp["k"]
    searching = inp["mode"] != DOTS
    plan = searching and inp["has_plan"]
    budget = int(env.get("SGPU_LDS_TARGET", BUDGET))
    qn_want = max(4, inp["max_nnz"]) if reading == "qn_unrounded" else max(4, (inp["max_nnz"] + 3) & ~3)
    need(o["qn"] == qn_want, "qn %d, the longest query rounded up to 4 is %d" % (o["qn"], qn_want))
    qn, qc, qg = o["qn"], o["qc"], o["qg"]
    need(qc == max(1, 1 if not searching else min(inp["query_cut"], qn)), "qc %d" % qc)
    need(o["p_query_cut"] == (1 if not searching else min(inp["query_cut"], qn)), "query_cut %d" % o["p_query_cut"])
    # ---- layout: what the kernel reads from each area, in the documented order
    sorted_first = bool(inp["first_sorted"]) and plan
    lookup_bytes = {PACKED: up((inp["dim"] // 32 + 1) * 8), DENSE: up(inp["dim"] + 1),
                    SPLIT: up((inp["dim"] // 32 + 1) * 4) + up((inp["dim"] // 32 + 1) * 2), HASH: 4096 * 8}[o["lookup"]] if searching else 0
    areas = [("q_sc", (qn + 1) * 4)]
    if inp["value_type"] != F16:
        areas.append(("q_val", (qn + 1) * 4))
    areas += [("q_comp", qn * 4), ("sel", (6 * qc + 1) * 4), ("rt_start", qg * qn * 8), ("rt_mid", qg * qn * 2),
              ("rt_pre", 2 * qg * (qn + 1) * 4), ("dots", o["dots_cap"] * 4), ("order", inp["max_nb"] * 2 if sorted_first else 0),
              ("part", 2 * (NT // 64 + 1) * 4), ("heap", kr * 64 * 8), ("st", 160 * 4), ("q_bits", lookup_bytes), ("uni", 0)]
    need(o["q_sc"] == 0, "q_sc is not kQscOffset")
    need((o["q_val"] != o["q_sc"]) == (inp["value_type"] != F16), "q_val / q_sc for value type %d" % inp["value_type"])
    for (a, size), (b, _) in zip(areas, areas[1:]):
        need(o[a] % 16 == 0 and o[b] % 16 == 0, "%s / %s not on 16 bytes" % (a, b))
        need(o[a] + size <= o[b], "%s (%d bytes at %d) overlaps %s at %d" % (a, size, o[a], b, o[b]))
    need(o["q_bits"] <= o["q_rank"] <= o["uni"] and o["q_rank"] % 16 == 0, "q_rank outside the lookup table")
    lds_limit = min(inp["max_lds"] or 65536, 160 * 1024)
    need(o["total"] == o["lds_bytes"] <= lds_limit and o["total"] % 16 == 0, "total %d, lds %d" % (o["total"], o["lds_bytes"]))
    need(o["uni"] <= o["total"], "union region starts past the end")
    uni_bytes = o["lds_bytes"] - o["uni"]
    if sorted_first and inp["max_nb"] > 1:       # the sort keys of the first list: 8 bytes x the next power of two
        need(uni_bytes >= 8 << (inp["max_nb"] - 1).bit_length(), "sort keys do not fit the union region")
    if plan:
        need(o["dots_cap"] >= inp["max_list_nb"], "dots area smaller than the largest list")
    need(1 <= qg <= qc, "qg %d of %d" % (qg, qc))
    if plan and "SGPU_LIST_GROUP" not in env:
        # everything but row tables and dots, as the layout has it (order .. st), the lookup table by the index's shape,
        # a union region of 512 items
        tail = o["q_bits"] - o["order"]
        if reading == "rest_without_heap":
            tail -= up(kr * 64 * 8)
        dense_shape = inp["comp_width"] == 2 and inp["dim"] <= 65535 and inp["max_nnz"] <= 255
        rest = tail + (up(inp["dim"] + 1) if dense_shape else up((inp["dim"] // 32 + 1) * 6)) + up(512 * 16 + NT * 12)
        rt_all = up(qc * qn * 8) + up(qc * qn * 2) + up(2 * qc * (qn + 1) * 4)
        exceeds = o["rt_start"] + rt_all + rest + inp["dots_cap"] * 4 > budget
        need(qg == (4 if exceeds and qc > 4 else qc), "lists per group %d of %d, budget exceeded: %s" % (qg, qc, exceeds))
    # ---- variant
    counted, coop, streamed = bool(o["counted"]), o["coop"] != 0, bool(o["streamed"])
    need(variant_built(NT, kr, counted, coop, streamed), "variant %s is not built" % ((NT, kr, counted, coop, streamed),))
    need(not (coop and streamed), "cooperative and streamed")
    need(counted == (inp["mode"] == COUNTED or bool(int(env.get("SGPU_VISITED_BITMAP", 0)))), "counted")
    families = ({PACKED, DENSE} if inp["comp_width"] == 2 else
                {PACKED, SPLIT} if inp["value_type"] == FIXEDU8 else {PACKED, SPLIT, HASH})
    need(o["lookup"] in families, "lookup %d for comp_width %d, value type %d" % (o["lookup"], inp["comp_width"], inp["value_type"]))
    if o["lookup"] == DENSE:
        need(inp["dim"] <= 65535 and inp["max_nnz"] <= 255, "dense byte table for this vocabulary / query")
    if o["lookup"] == SPLIT:
        need(inp["max_nnz"] <= 65535, "16-bit ranks for a longer query")
    if o["lookup"] == HASH:
        need(inp["hash_ok"] and inp["dim"] <= 1 << 24, "hashed lookup without seeds")
    if NT == 1024 and "SGPU_BLOCK" not in env:
        need(inp["nq"] <= inp["n_cu"], "1024 threads for more queries than CUs")
    if NT == 1024:
        need(not counted and k <= 128, "1024 threads: counted %s, k %d" % (counted, k))
    # who may be cooperative at all
    mode_coop = env.get("SGPU_COOP")
    if reading == "coop_ignores_broken":
        may = inp["mode"] == SEARCH and not counted and mode_coop != "0"
    else:
        may = inp["mode"] == SEARCH and not counted and mode_coop != "0" and not inp["coop_broken"]
    n_cu, nq = inp["n_cu"], inp["nq"]
    by_size = nq <= n_cu * 11 // 16 or n_cu < nq <= n_cu * 7 // 4
    if "SGPU_COOP_MAX_NQ" in env:
        by_size = nq <= int(env["SGPU_COOP_MAX_NQ"])
    want_coop = may and (mode_coop == "force" or by_size) and variant_built(NT, kr, False, True, False)
    need(coop == want_coop, "cooperative %d, the rule says %s" % (o["coop"], want_coop))
    need(o["coop"] == (2 if coop and mode_coop == "force" else int(coop)), "forced flag")
    need(o["ring"] == o["p_ring"] and (o["ring"] != 0) == streamed, "ring %d, streamed %s" % (o["ring"], streamed))
    need(o["items_min"] <= o["items_init"], "items_min %d > items_init %d" % (o["items_min"], o["items_init"]))
    if streamed:
        ring = o["ring"]
        need(ring in (256, 512, 1024), "ring %d" % ring)
        if reading == "ring_unrounded" and "SGPU_RING_MAX" in env:
            need(ring == min(1024, max(256, int(env["SGPU_RING_MAX"]))), "ring %d is not SGPU_RING_MAX" % ring)
        need(ring <= max(256, int(env.get("SGPU_RING_MAX", 1024))), "ring %d above SGPU_RING_MAX" % ring)
        need(ring_bytes(ring) <= uni_bytes, "ring of %d slots in %d bytes" % (ring, uni_bytes))
        need(o["dots_cap"] <= 65535, "16-bit dot indices")
        need(o["items_max"] % 128 == 0 and 128 <= o["items_max"] <= 1024, "items_max %d" % o["items_max"])
        need(o["items_max"] * 16 + NT * 12 <= uni_bytes, "refinement round of %d items in %d bytes" % (o["items_max"], uni_bytes))
        need(o["items_init"] <= max(o["items_max"], ring), "items_init %d" % o["items_init"])
    else:
        need(o["items_max"] * 16 + NT * 12 <= uni_bytes or not searching, "round of %d items in %d bytes" % (o["items_max"], uni_bytes))
        need(o["items_init"] <= o["items_max"], "items_init %d > items_max %d" % (o["items_init"], o["items_max"]))
    if coop:
        need(uni_bytes >= 4096, "helpers' tables")
        need(1 <= o["chunk_min"] <= o["chunk"] <= min(NT, 1023), "chunk %d .. %d" % (o["chunk_min"], o["chunk"]))
        need(o["max_cand"] * 20 <= uni_bytes and o["chunk"] * 16 <= uni_bytes, "candidates / chunk tables")
        need(o["max_cand"] <= NT and 1 <= o["max_pos"] <= 65535 and o["max_pos"] >= min(o["dots_cap"], 65535), "max_cand / max_pos")
        need(o["poll_sleep"] >= 1 and o["first_reach"] >= 1, "poll / first reach")
        occ = inp["occupancy_grid"]
        if occ:
            g = occ
            most = int(env["SGPU_COOP_GRID"]) if "SGPU_COOP_GRID" in env else max((48 + 32 * nq) * n_cu // 256, 8)
            if o["coop"] == 1 and most:
                g = max(min(occ, most), min(nq, occ))
            need(o["grid"] == min(g, 512), "cooperative grid %d, the rule gives %d" % (o["grid"], min(g, 512)))
            # the board: [open 64 | counters 64 | 8 words per slot | max_pos x 8 per slot | max_cand x 16 per slot | trace]
            G = o["grid"]
            need(o["board_slots"] == 128 and o["board_pos"] >= 128 + G * 64 and o["board_cand"] >= o["board_pos"] + G * o["max_pos"] * 8 and
                 o["board_trace"] >= o["board_cand"] + G * o["max_cand"] * 16 and o["board_total"] >= o["board_trace"] + G * 128, "board")
    elif inp["occupancy_grid"]:
        need(o["grid"] == max(1, min(inp["occupancy_grid"], nq)), "plain grid %d" % o["grid"])
    need(o["p_k"] == k and o["p_mode"] == (DOTS if inp["mode"] == DOTS else SEARCH) and 1 <= o["rblocks_max"] <= 32, "kernel parameters")
    need(o["target_list"] == (inp["query_cut"] if inp["mode"] == DOTS else 0), "target list")
    return bad


def ok(monkeypatch, env=None, **facts):
    inp, out = configure(monkeypatch, env, **facts)
    bad = violations(inp, out, env)
    assert not bad, (facts, env, bad, out)
    return out


def fails(monkeypatch, status, text, env=None, heap_factor=1.0, **facts):
    with pytest.raises(SeismicHipError) as e:
        configure(monkeypatch, env, heap_factor, **facts)
    assert e.value.status == status and text in str(e.value), str(e.value)


# ---- rows -----------------------------------------------------------------------------------------------------------
U16 = dict(comp_width=2, dim=30522)                      # the benchmark's vocabulary: the dense byte table
U32 = dict(comp_width=4, dim=200000, hash_ok=1)
U32_BIG = dict(comp_width=4, dim=400000, hash_ok=0)      # 100 KB of packed words, 75 KB split


@pytest.mark.parametrize("k", [1, 10, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
@pytest.mark.parametrize("nq", [1, 176, 177, 256, 257, 448, 449, 10000])
def test_heap_sizes_and_launch_sizes(monkeypatch, k, nq):
    """k at every heap variant's edge x nq at the edges of coop_by_size's two windows (n_cu 11/16, n_cu, n_cu 7/4) and a
    throughput batch: variant, workgroup size, grid."""
    out = ok(monkeypatch, k=k, nq=nq, dots_cap=900, max_list_nb=300, occupancy_grid=512, **U16)
    assert out["block"] == (1024 if nq <= N_CU and k <= 128 else 512)
    assert (out["coop"] != 0) == ((nq <= 176 or 257 <= nq <= 448) and k <= 256)
    assert out["lookup"] == DENSE


@pytest.mark.parametrize("max_nnz", [0, 1, 255, 256, 65535, 65536])
@pytest.mark.parametrize("idx", [U16, U32, dict(U16, value_type=FIXEDU8), dict(U32, value_type=FIXEDU8), dict(U16, value_type=DOTVBYTE)])
def test_query_lengths(monkeypatch, max_nnz, idx):
    facts = dict(idx, max_nnz=max_nnz, nq=1000, query_cut=1)
    try:
        out = ok(monkeypatch, **facts)
    except SeismicHipError as e:      # 64K components: the weights alone are 256 KB (x 2 for u8 values) - a named limit, not a layout
        assert e.status == ELIMIT and max_nnz >= 65535, str(e)
        return
    assert max_nnz < 65535 and out["qn"] % 4 == 0
    if idx["comp_width"] == 2:
        assert out["lookup"] == (DENSE if max_nnz <= 255 else PACKED)


@pytest.mark.parametrize("dim", [65535, 65536, (1 << 24) - 1, (1 << 24) + 1])
def test_vocabulary_sizes(monkeypatch, dim):
    """u32 components: the hashed entries serve any vocabulary below 2^24 (24-bit multiply); the bit tables of a 2^24
    vocabulary are megabytes - a named limit. u16 components: the dense byte table up to 65535."""
    if dim < 1 << 24:
        assert ok(monkeypatch, comp_width=4, dim=dim, hash_ok=1, nq=1000)["lookup"] == HASH
    else:
        fails(monkeypatch, ELIMIT, "-word bitmap", comp_width=4, dim=dim, hash_ok=0, nq=1000)
    if dim <= 65536:
        small = ok(monkeypatch, comp_width=4, dim=dim, hash_ok=0, nq=1000)
        assert small["lookup"] == PACKED and small["q_rank"] == small["q_bits"] + up((dim // 32 + 1) * 8) == small["uni"]
    if dim <= 65535:
        assert ok(monkeypatch, comp_width=2, dim=dim, nq=1000)["lookup"] == DENSE


@pytest.mark.parametrize("query_cut", [0, 1, 4, 5, 16, 17, 100])
def test_query_cuts(monkeypatch, query_cut):
    """0 walks no list (one slot kept), > qn is clamped; groups of lists from 5 on when the budget says so."""
    out = ok(monkeypatch, query_cut=query_cut, max_nnz=30, nq=1000, dots_cap=200 * max(query_cut, 1), max_list_nb=200, **U16)
    assert out["qc"] == max(1, min(query_cut, 32)) and out["p_query_cut"] == min(query_cut, 32)
    big = ok(monkeypatch, query_cut=query_cut, max_nnz=160, nq=1000, dots_cap=5000, max_list_nb=900, **U16)
    assert big["qg"] == (4 if query_cut > 4 else big["qc"]), big     # 20 KB of dots, the dense table, 160 components: groups of four


@pytest.mark.parametrize("max_nb", [0, 1, 2, 1000, 1024, 1025])
def test_sorted_first_list(monkeypatch, max_nb):
    out = ok(monkeypatch, first_sorted=1, max_nb=max_nb, dots_cap=max(1, 3 * max_nb), max_list_nb=max(1, max_nb), nq=1000, **U16)
    unsorted = ok(monkeypatch, first_sorted=0, max_nb=max_nb, dots_cap=max(1, 3 * max_nb), max_list_nb=max(1, max_nb), nq=1000, **U16)
    assert out["part"] - out["order"] == up(2 * max_nb) and unsorted["part"] == unsorted["order"]
    assert out["p_first_sorted"] == 1 and unsorted["p_first_sorted"] == 0


def test_dots_beyond_24_kib_shrink_to_what_fits_but_never_below_the_largest_list(monkeypatch):
    out = ok(monkeypatch, nq=1000, query_cut=10, dots_cap=36000, max_list_nb=3600, **U16)
    assert 6144 <= out["dots_cap"] < 36000 and out["lds_bytes"] <= BUDGET
    out = ok(monkeypatch, nq=1000, query_cut=10, dots_cap=36000, max_list_nb=20000, **U16)
    assert out["dots_cap"] == 20000 and out["lds_bytes"] > BUDGET
    out = ok(monkeypatch, nq=1000, query_cut=10, dots_cap=6144, max_list_nb=100, **U16)      # exactly 24 KiB: left alone
    assert out["dots_cap"] == 6144
    out = ok(monkeypatch, {"SGPU_DOTS_CAP": 50}, nq=1000, query_cut=10, dots_cap=6144, max_list_nb=100, **U16)
    assert out["dots_cap"] == 100


def test_what_cannot_fit_says_which_part(monkeypatch):
    fails(monkeypatch, ELIMIT, "do not fit the row tables in LDS", nq=1000, query_cut=64, max_nnz=4096, **U16)
    fails(monkeypatch, ELIMIT, "before its lookup table", nq=1000, query_cut=4, dots_cap=60000, max_list_nb=41000, **U16)
    fails(monkeypatch, ELIMIT, "lower query_cut / use first_sorted=0", nq=1000, query_cut=4, dots_cap=37000, max_list_nb=37000, **U16)
    fails(monkeypatch, ELIMIT, "lower query_cut / use first_sorted=0", nq=1000, max_lds=65536, dots_cap=12000, max_list_nb=12000, **U16)


def test_bad_arguments(monkeypatch):
    fails(monkeypatch, EINVAL, "k must be > 0", k=0)
    fails(monkeypatch, EINVAL, "exceeds the batch's k_max", k=11, k_max=10)
    fails(monkeypatch, EINVAL, "heap_factor is NaN", heap_factor=float("nan"))
    fails(monkeypatch, EINVAL, "SGPU_BLOCK must be 512 or 1024", env={"SGPU_BLOCK": 256})
    ok(monkeypatch, heap_factor=-1.0)
    ok(monkeypatch, heap_factor=float("inf"))


def test_other_modes(monkeypatch):
    out = ok(monkeypatch, mode=COUNTED, nq=8, **U16)
    assert out["counted"] == 1 and out["block"] == 512 and out["coop"] == 0 and out["streamed"] == 0
    out = ok(monkeypatch, mode=DOTS, has_plan=0, query_cut=7, target_list_nb=3000, k=1, k_max=1, nq=1, **U16)
    assert out["dots_cap"] == 3000 and out["block"] == 512 and out["q_bits"] == out["uni"] and out["qc"] == 1
    out = ok(monkeypatch, mode=DOTS, has_plan=0, query_cut=7, target_list_nb=0, k=1, k_max=1, nq=1, **U16)
    assert out["dots_cap"] == 1
    out = ok(monkeypatch, staged=1, nq=3, **U16)
    assert out["queue_base"] == 0
    assert ok(monkeypatch, coop_broken=1, nq=3, **U16)["coop"] == 0
    assert ok(monkeypatch, max_lds=0, nq=3, **U16)["lds_bytes"] <= 65536


FORCING = [
    ({"SGPU_FORCE_DENSE": 1}, dict(U16, nq=1000, dots_cap=5000, max_list_nb=5000), dict(lookup=DENSE)),
    ({"SGPU_NO_DENSE": 1}, dict(U16, nq=1000), dict(lookup=PACKED)),
    ({"SGPU_FORCE_SPLIT": 1}, dict(U32, nq=1000), dict(lookup=SPLIT)),
    ({"SGPU_NO_SPLIT": 1}, dict(U32_BIG, nq=1000), dict(lookup=PACKED)),
    ({}, dict(U32_BIG, nq=1000), dict(lookup=SPLIT)),
    ({}, dict(U32, nq=1000), dict(lookup=HASH)),
    ({"SGPU_NO_HASH": 1}, dict(U32, nq=1000), dict(lookup=PACKED)),
    ({"SGPU_NO_LPT": 1}, dict(U32, nq=1000), dict(lookup=PACKED)),
    ({"SGPU_FORCE_HASH": 1}, dict(U32, nq=1000, dots_cap=6144, max_list_nb=6144), dict(lookup=HASH)),
    ({"SGPU_ITEMS_MAX": 256}, dict(U16, nq=1000), dict(ring=256, lookup=DENSE)),
    ({"SGPU_ITEMS_MAX": 384, "SGPU_STREAM": 0}, dict(U16, nq=1000), dict(items_max=384, streamed=0, ring=0)),
    ({"SGPU_ITEMS_MAX": ""}, dict(U16, nq=1000), dict(ring=1024)),
    ({"SGPU_ITEMS_INIT": 32}, dict(U16, nq=1), dict(items_init=32)),
    ({"SGPU_RING_MAX": 700}, dict(U16, nq=1000), dict(ring=512, streamed=1)),
    ({"SGPU_RING_MAX": 100}, dict(U16, nq=1000), dict(ring=256)),
    ({"SGPU_RING_MAX": 4096}, dict(U16, nq=1000), dict(ring=1024)),
    ({"SGPU_DOTS_CAP": 64}, dict(U16, nq=1000, dots_cap=900, max_list_nb=40), dict(dots_cap=64)),
    ({"SGPU_LDS_TARGET": 40000}, dict(U16, nq=1000, query_cut=8, max_nnz=64), dict(lookup=PACKED, qg=4)),
    ({"SGPU_LIST_GROUP": 2}, dict(U16, nq=1000, query_cut=8), dict(qg=2)),
    ({"SGPU_LIST_GROUP": 0}, dict(U16, nq=1000, query_cut=8), dict(qg=1)),
    ({"SGPU_BLOCK": 512}, dict(U16, nq=1), dict(block=512)),
    ({"SGPU_BLOCK": 1024}, dict(U16, nq=1000), dict(block=1024)),
    ({"SGPU_BLOCK": 1024}, dict(U16, nq=1000, k=129), dict(block=512)),
    ({"SGPU_COOP": "0"}, dict(U16, nq=1), dict(coop=0, streamed=1)),
    ({"SGPU_COOP": "force"}, dict(U16, nq=1000, occupancy_grid=512), dict(coop=2, streamed=0, idle_min=0, idle_ratio=0, grid=512)),
    ({"SGPU_COOP": "force"}, dict(U16, nq=1000, k=257), dict(coop=0, streamed=1)),
    ({"SGPU_COOP_MAX_NQ": 256}, dict(U16, nq=200), dict(coop=1)),
    ({"SGPU_COOP_MAX_NQ": 256}, dict(U16, nq=300), dict(coop=0)),
    ({"SGPU_COOP_GRID": 0}, dict(U16, nq=1, occupancy_grid=256), dict(grid=256)),
    ({"SGPU_COOP_GRID": 16}, dict(U16, nq=1, occupancy_grid=256), dict(grid=16)),
    ({"SGPU_STREAM": 0}, dict(U16, nq=1000), dict(streamed=0, ring=0)),
    ({"SGPU_VISITED_BITMAP": 1}, dict(U16, nq=1), dict(counted=1, block=512, coop=0)),
    ({"SGPU_COOP_CHUNK": 5000, "SGPU_COOP_CHUNK_MIN": 0}, dict(U16, nq=1), dict(chunk=1023, chunk_min=1)),
]


@pytest.mark.parametrize("env,facts,want", FORCING, ids=lambda x: None)
def test_forcing_hooks(monkeypatch, env, facts, want):
    out = ok(monkeypatch, env, **facts)
    assert {n: out[n] for n in want} == want, out


def test_cooperative_grid_rule(monkeypatch):
    """48 + 32 per query scaled by n_cu / 256, never fewer workgroups than queries (or than fit), capped at the board's 512."""
    for n_cu, nq, occ, want in [(256, 1, 256, 80), (256, 2, 512, 112), (256, 8, 512, 304), (256, 100, 512, 512), (256, 176, 256, 256),
                                (256, 300, 512, 512), (256, 300, 768, 512), (128, 1, 256, 40), (64, 1, 128, 20), (8, 1, 16, 8),
                                (304, 1, 608, 95), (256, 40, 32, 32)]:
        out = ok(monkeypatch, n_cu=n_cu, nq=nq, occupancy_grid=occ, **U16)
        assert out["coop"] == 1 and out["grid"] == want, (n_cu, nq, occ, out["grid"])
    assert ok(monkeypatch, nq=200, occupancy_grid=512, **U16)["grid"] == 200      # plain: one workgroup per query at most
    assert ok(monkeypatch, nq=5000, occupancy_grid=512, **U16)["grid"] == 512


def test_cooperative_windows_on_another_chip(monkeypatch):
    n_cu = 304
    for nq, want in [(304 * 11 // 16, 1), (304 * 11 // 16 + 1, 0), (304, 0), (305, 1), (304 * 7 // 4, 1), (304 * 7 // 4 + 1, 0)]:
        assert ok(monkeypatch, n_cu=n_cu, nq=nq, **U16)["coop"] == want, nq


def test_a_latency_bound_cooperative_launch_bootstraps_with_one_local_round(monkeypatch):
    assert ok(monkeypatch, nq=1, **U16)["items_init"] == 128
    assert ok(monkeypatch, {"SGPU_COOP_ITEMS_INIT": 512}, nq=1, **U16)["items_init"] == 512
    assert ok(monkeypatch, {"SGPU_COOP_ITEMS_INIT": 512, "SGPU_ITEMS_INIT": 64}, nq=1, **U16)["items_init"] == 64
    assert ok(monkeypatch, {"SGPU_COOP_ITEMS_INIT": 512}, nq=300, **U16)["items_init"] == 128


def test_without_the_switch_the_hook_is_inert_and_hooks_are_ignored(monkeypatch):
    inp, want = configure(monkeypatch, nq=1000, **U16)
    monkeypatch.setenv("SGPU_TEST_HOOKS", "0")
    with pytest.raises(SeismicHipError) as e:
        debug_launch_config(nq=1000, **U16)
    assert e.value.status == EINVAL and "is a test hook" in str(e.value)


# ---- wrong readings of the contract: each must fail on a named row, and only there ------------------------------------
def _seen(monkeypatch, reading, env=None, **facts):
    inp, out = configure(monkeypatch, env, **facts)
    assert not violations(inp, out, env), (facts, violations(inp, out, env))
    return violations(inp, out, env, reading)


def test_a_rest_that_forgets_the_heap_is_seen(monkeypatch):
    # k = 1024: 8 KB of heap. Five lists x 64 components, 10 000 block dots and the dense table pass the budget only with it
    row = dict(U16, nq=1000, k=1024, query_cut=5, max_nnz=64, dots_cap=5500, max_list_nb=1100)
    assert any("lists per group" in v for v in _seen(monkeypatch, "rest_without_heap", **row))
    assert _seen(monkeypatch, "rest_without_heap", **dict(row, dots_cap=100, max_list_nb=100)) == []     # far from the budget


def test_a_ring_that_is_not_rounded_down_to_a_power_of_two_is_seen(monkeypatch):
    assert any("SGPU_RING_MAX" in v for v in _seen(monkeypatch, "ring_unrounded", {"SGPU_RING_MAX": 700}, nq=1000, **U16))
    assert _seen(monkeypatch, "ring_unrounded", {"SGPU_RING_MAX": 512}, nq=1000, **U16) == []


def test_a_cooperative_wish_that_ignores_coop_broken_is_seen(monkeypatch):
    assert any("cooperative" in v for v in _seen(monkeypatch, "coop_ignores_broken", nq=1, coop_broken=1, **U16))
    assert _seen(monkeypatch, "coop_ignores_broken", nq=1000, coop_broken=1, **U16) == []                 # (plain by size anyway)


def test_a_qn_that_is_not_rounded_to_four_is_seen(monkeypatch):
    for max_nnz in (5, 255, 30):
        assert any("rounded up to 4" in v for v in _seen(monkeypatch, "qn_unrounded", nq=1000, max_nnz=max_nnz, **U16)), max_nnz
    for max_nnz in (0, 1, 4, 256):
        assert _seen(monkeypatch, "qn_unrounded", nq=1000, max_nnz=max_nnz, **U16) == [], max_nnz
