"""The launch configuration the test hook reports (sgpu_debug_launch_config, no device) is the one real launches take:
for a handful of launches - 1, n_cu and n_cu + 1 queries, k in three heap variants, f16 / fixed-u8 / DotVByte indexes with
u16 components and a fixed-u8 one with u32 components, a counted pass, a MODE_DOTS call - the hook is fed the facts the
launch had (the plan's numbers from sgpu_debug_plan) and its workgroup size and LDS bytes are compared with the launch's
sgpu_launch_stats; the grid with the hook's rule at the occupancies a CU can have. Indexes whose lookup family does not
depend on the per-query hash seeds (which no entry point reports) are used throughout."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig, LaunchStats
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu
DIM = 512
FIXEDU8, DOTVBYTE = 1, 2


@functools.lru_cache(maxsize=None)
def _index(comp_width, value_type):
    off, comps, vals = random_dataset(5, 3000, DIM, nnz_lo=8, nnz_hi=120)
    ix = _native.NativeIndex.build(comp_width, DIM, off, comps, vals,
                                   BuildConfig.defaults(n_postings=100, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0))
    if value_type:
        ix = ix.convert(value_type)
    ix.upload(0)
    return ix


def _chip():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count, int(getattr(p, "shared_memory_per_block", 160 * 1024))


def _plan(ix, q, cut):
    q_off, qc, qv = (np.ascontiguousarray(a, t) for a, t in zip(q, (np.uint64, np.uint32, np.float32)))
    nq = len(q_off) - 1
    order, out3 = np.zeros(max(nq, 1), np.uint32), np.zeros(3, np.uint32)
    vp = ctypes.c_void_p
    fn = _native.lib().sgpu_debug_plan
    fn.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    _native.check(fn(ix.h, *(a.ctypes.data_as(vp) for a in (q_off, qc, qv)), nq, cut, order.ctypes.data_as(vp), out3.ctypes.data_as(vp)))
    return dict(dots_cap=int(out3[0]), max_nb=int(out3[1]), max_list_nb=int(out3[2]))


def _agrees(stats, facts):
    n_cu, max_lds = _chip()
    grids = set()
    for per_cu in range(1, 9):
        out = _native.debug_launch_config(n_cu=n_cu, max_lds=max_lds, occupancy_grid=n_cu * per_cu, **facts)
        grids.add(out["grid"])
    print("launch", facts, "->", stats.n_queries, stats.grid, stats.block, stats.lds_bytes, "hook", out["block"], out["lds_bytes"], sorted(grids))
    assert (stats.block, stats.lds_bytes) == (out["block"], out["lds_bytes"]), (facts, out)
    assert stats.grid in grids, (facts, stats.grid, grids)
    return out


def _search_facts(ix, comp_width, value_type, q, k, cut, **more):
    max_nnz = int(np.diff(q[0]).max())
    qn = max(4, (max_nnz + 3) & ~3)
    return dict(comp_width=comp_width, value_type=value_type, dim=DIM, nq=len(q[0]) - 1, max_nnz=max_nnz, k_max=k, k=k, query_cut=cut,
                has_plan=1, hash_ok=0, **_plan(ix, q, min(cut, qn)), **more)


@pytest.mark.parametrize("k", [10, 129, 257])
def test_f16_launches_of_one_n_cu_and_n_cu_plus_one_queries(k):
    ix, n_cu = _index(2, 0), _chip()[0]
    for nq in (1, n_cu, n_cu + 1):
        q = random_queries(6 + nq, nq, DIM, 5, 50)
        stats = _native.DeviceBatch(ix, *q, k).run(k, 4, 1.0)
        out = _agrees(stats, _search_facts(ix, 2, 0, q, k, 4))
        assert out["block"] == (1024 if nq <= n_cu and k <= 128 else 512)
        assert (out["coop"] != 0) == (nq != n_cu and k <= 256)      # (1 query and the window past n_cu; k > 256 has no variant)


@pytest.mark.parametrize("comp_width,value_type", [(2, FIXEDU8), (2, DOTVBYTE), (4, FIXEDU8)])
def test_the_other_record_formats(comp_width, value_type):
    ix, n_cu = _index(comp_width, value_type), _chip()[0]
    for nq, cut, first_sorted in ((1, 4, 0), (n_cu + 1, 4, 0), (2000, 9, 1)):
        q = random_queries(16 + nq, nq, DIM, 5, 50)
        stats = _native.DeviceBatch(ix, *q, 10).run(10, cut, 0.9, first_sorted=bool(first_sorted))
        out = _agrees(stats, _search_facts(ix, comp_width, value_type, q, 10, cut, first_sorted=first_sorted))
        assert out["q_val"] != out["q_sc"]
        if nq == 2000:      # a plain launch larger than the chip: the grid IS the occupancy - and the hook's grid at that occupancy
            assert stats.grid % n_cu == 0 and out["coop"] == 0 and out["streamed"] == 1


def test_a_counted_pass():
    ix = _index(2, 0)
    q = random_queries(3, 40, DIM, 5, 50)
    stats = _native.DeviceBatch(ix, *q, 10).run_counted(10, 4, 1.0)
    out = _agrees(stats, _search_facts(ix, 2, 0, q, 10, 4, mode=2))
    assert out["counted"] == 1 and out["block"] == 512 and stats.grid == 40


def test_a_summary_distances_call():
    ix = _index(2, 0)
    lbs = orc.desc_arrays(ix.desc)["list_block_start"].astype(np.int64)
    lst = int(np.argmax(np.diff(lbs)))
    _, qc, qv = random_queries(9, 1, DIM, 20, 20)
    ix.summary_distances(lst, qc, qv)
    stats = LaunchStats()
    _native.check(_native.lib().sgpu_batch_sync(ix.h, ctypes.byref(stats)))
    out = _agrees(stats, dict(comp_width=2, value_type=0, dim=DIM, nq=1, max_nnz=len(qc), k_max=1, k=1, query_cut=lst, has_plan=0,
                              target_list_nb=int(lbs[lst + 1] - lbs[lst]), mode=1))
    assert out["block"] == 512 and stats.grid == 1 and out["dots_cap"] == int(lbs[lst + 1] - lbs[lst])
