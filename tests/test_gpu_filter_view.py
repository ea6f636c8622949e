"""A filter's device view, posting for posting. DESIGN.md ("Document filters") rests filtered search on the view claim:
block_post_start', post_ref' and post_doc' are the postings of allowed documents in their original order within each
block, knn' the graph with the neighbours outside the set masked. Here the view is read back from the device
(sgpu_debug_posting_view) and EVERY element of every array is compared with a numpy compaction of the replica's own
arrays (filter_cases.expected_view), on cases whose posting counts and kept-posting patterns sit on the edges of the
kernels that build it (tests/filter_cases.py; what the cases can see: tests/test_filter_cases_cpu.py). A mismatch names the
array, the first differing index, its tile, word and lane and the two values. Run with `-m gpu`."""
import time

import numpy as np
import pytest

import filter_cases as FC
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from test_gpu_filter import FilteredDesc, _same
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu


def _base(ix, replica=0):
    """The replica's own arrays read back; what the host knows of them is asserted on the way."""
    base = ix.debug_posting_view(replica)
    a = orc.desc_arrays(ix.desc)
    assert np.array_equal(base["block_post_start"], a["block_post_start"].astype(np.uint32))
    assert np.array_equal(base["post_doc"], a["post_doc"]) and len(base["post_ref"]) == len(base["post_doc"])
    assert set(base) == {"block_post_start", "post_ref", "post_doc", "knn"}
    return base


def _assert_view(ix, f, allowed, base, what, replica=0):
    got = f.debug_view(replica)
    diff = FC.view_diff(got, FC.expected_view(base, allowed, int(ix.desc.n_docs)))
    assert diff is None, "%s: %s" % (what, diff)
    return got


def _all_sets(ix, what, single=True, names=None, replica=0):
    """Every allowed set of the index against the expectation from the replica's base; returns the kept postings per set."""
    base = _base(ix, replica)
    sets = FC.allowed_sets(ix.desc, base["post_doc"], names=names)
    kept = FC.check_sets(sets, base["post_doc"], single=single)
    for name, (allowed, _) in sets.items():
        f = ix.make_filter(allowed)
        assert f.count == int(allowed.sum())
        _assert_view(ix, f, allowed, base, "%s, set %s" % (what, name), replica)
        assert f.device_bytes() > 0
        f.close()
    return base, sets, kept


@pytest.fixture(scope="module")
def blocks():
    case = FC.make("blocks")
    ix = case.build()
    case.check(ix.desc)
    return case, ix


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_every_small_case_under_every_allowed_set(name):
    case = FC.make(name)
    ix = case.build()
    print("filter case %s: %s -> %s" % (name, case.paths, case.check(ix.desc)))
    ix.upload(0)
    base, sets, kept = _all_sets(ix, name)
    print("kept postings per set:", kept)
    if name == "exact_0":       # the n_p == 0 branch: n_blocks + 1 zeros
        for allowed, _ in sets.values():
            v = ix.make_filter(allowed).debug_view()
            assert len(v["block_post_start"]) == int(ix.desc.n_blocks) + 1 and not v["block_post_start"].any()
            assert len(v["post_doc"]) == 0 and len(v["post_ref"]) == 0


@pytest.mark.parametrize("knn_dim", [0, 1, 6])
def test_the_masked_graph(blocks, knn_dim):
    """The blocks case with a seeded random graph of 1 and of 6 neighbours per document, and without one - then the view
    has the base's graph, that is none. sgpu_index_set_knn rejects ids >= n_docs, so the `d < n_docs` arm of
    filter_knn_kernel cannot be reached through the API: it is not run here (what an id >= n_docs must become is
    restated and checked against a wrong reading in test_filter_cases_cpu.py)."""
    case, _ = blocks
    ix = case.build().upload(0)
    if knn_dim:
        graph = np.random.default_rng(40 + knn_dim).integers(0, case.n_docs, case.n_docs * knn_dim).astype(np.uint32)
        ix.set_knn(graph, knn_dim)
        with pytest.raises(_native.SeismicHipError):
            ix.set_knn(np.full(case.n_docs * knn_dim, case.n_docs, np.uint32), knn_dim)
    base, sets, _ = _all_sets(ix, "blocks, knn_dim %d" % knn_dim)
    if knn_dim:
        assert np.array_equal(base["knn"], graph)
    else:
        assert len(base["knn"]) == 0
        assert len(ix.make_filter(sets["p50"][0]).debug_view()["knn"]) == 0


def test_forward_layouts(monkeypatch):
    """post_ref differs between the block-major and the document-major forward store; post_ref' follows its own upload."""
    for name in ("exact_65", "blocks"):
        case = FC.make(name)
        refs = {}
        for layout in ("block", "doc"):
            monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)
            ix = case.build().upload(0)
            base, _, _ = _all_sets(ix, "%s, layout %s" % (name, layout))
            refs[layout] = base["post_ref"]
        assert len(refs["block"]) == len(refs["doc"]) and not np.array_equal(refs["block"], refs["doc"])
        assert np.array_equal(refs["block"] & np.uint64(0xffff), refs["doc"] & np.uint64(0xffff))     # (the length field)


@pytest.mark.parametrize("kind", ["fixedu8", "dotvbyte", "u32"])
def test_value_types_and_widths(blocks, kind):
    """post_ref carries the record's length and, for DotVByte, the raw bit: the 64-bit words come through unchanged."""
    if kind == "u32":
        dim = 70_000
        off, comps, vals = random_dataset(84, 1500, dim, nnz_lo=6, nnz_hi=60)
        ix = _native.NativeIndex.build(4, dim, off, comps, vals,
                                       BuildConfig.defaults(n_postings=40, centroid_fraction=0.2, summary_energy=0.5, max_fraction=4.0))
        single = False          # documents of several components: a set aimed at a posting keeps its document's others too
    else:
        ix = blocks[0].build().convert(1 if kind == "fixedu8" else 2)
        single = True
    ix.upload(0)
    base, _, kept = _all_sets(ix, kind, single=single)
    assert len(np.unique(base["post_ref"] >> np.uint64(16))) > 1 and kept["p50"] > 0


def test_replicas_and_generations(blocks):
    case, _ = blocks
    ix = case.build()
    ix.upload_many([0, 0])
    assert ix.replicas == 2
    bases = [_base(ix, r) for r in (0, 1)]
    sets = FC.allowed_sets(ix.desc, bases[0]["post_doc"], names=("holes", "p50", "lane63"))
    filters = {name: ix.make_filter(allowed) for name, (allowed, _) in sets.items()}
    for name, (allowed, _) in sets.items():
        for r in (0, 1):
            _assert_view(ix, filters[name], allowed, bases[r], "replica %d, set %s" % (r, name), r)
    with pytest.raises(_native.SeismicHipError) as e:
        filters["p50"].debug_view(2)
    assert e.value.status == 2                                   # SGPU_EDEVICE
    # a new upload, then a new graph: the view read back is the rebuilt one
    ix.upload(0)
    assert ix.replicas == 1
    base = _base(ix)
    for name, (allowed, _) in sets.items():
        _assert_view(ix, filters[name], allowed, base, "after a new upload, set %s" % name)
    with pytest.raises(_native.SeismicHipError):
        filters["p50"].debug_view(1)
    for seed, knn_dim in ((1, 3), (2, 3), (3, 2)):
        graph = np.random.default_rng(seed).integers(0, case.n_docs, case.n_docs * knn_dim).astype(np.uint32)
        ix.set_knn(graph, knn_dim)
        base = _base(ix)
        assert np.array_equal(base["knn"], graph)
        for name, (allowed, _) in sets.items():
            got = _assert_view(ix, filters[name], allowed, base, "after set_knn %d, set %s" % (seed, name))
            assert len(got["knn"]) == len(graph)


def test_the_view_read_back_is_the_view_searched(blocks):
    """Tie-in with search: filtered search on the index = plain search on an index made from the I_A descriptor."""
    case, _ = blocks
    ix = case.build().upload(0)
    base = _base(ix)
    allowed = FC.allowed_sets(ix.desc, base["post_doc"], names=("holes",))["holes"][0]
    f = ix.make_filter(allowed)
    q = random_queries(95, 64, case.dim, 2, 10)
    got = ix.batch_search(*q, 10, 4, 1.0, False, filter=f)
    view = _assert_view(ix, f, allowed, base, "holes, after the search")
    fd = FilteredDesc(ix.desc, allowed)
    assert np.array_equal(view["post_doc"], fd.post_doc) and np.array_equal(view["block_post_start"].astype(np.uint64), fd.bps)
    ia = _native.NativeIndex.from_desc(fd.desc).upload(0)
    _same(got, ia.batch_search(*q, 10, 4, 1.0, False))
    assert (got[2] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# the scan's second pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    case = FC.make("big")
    t0 = time.perf_counter()
    ix = case.build(use_device=1)
    t1 = time.perf_counter()
    ix.upload(0)
    t2 = time.perf_counter()
    found = case.check(ix.desc)
    base = _base(ix)
    sets = FC.allowed_sets(ix.desc, base["post_doc"], names=FC.BIG_SETS)
    FC.check_sets(sets, base["post_doc"])
    sides = FC.check_big_sets(sets, base["post_doc"])
    print("filter case big: %s -> %s; build %.2f s, upload %.2f s; kept postings before / from tile 4096: %s" % (
        case.paths, found, t1 - t0, t2 - t1, sides))
    return ix, base, sets


@pytest.mark.parametrize("name", FC.BIG_SETS)
def test_the_big_case_crosses_the_scans_pass_boundary(big, name):
    ix, base, sets = big
    allowed = sets[name][0]
    f = ix.make_filter(allowed)
    _assert_view(ix, f, allowed, base, "big, set %s" % name)
    f.close()
