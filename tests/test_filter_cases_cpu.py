"""The reference side of tests/test_gpu_filter_view.py, without a device: every case of tests/filter_cases.py has the
properties it exists for (check()), its allowed sets keep the postings they are aimed at, expected_view() agrees with
test_gpu_filter.FilteredDesc (the I_A the search tests hand to the oracle), and a numpy restatement of the device algorithm
- ballot words, tile counts, a scan in passes with a carry, a scatter by word prefix, a block remap with its two arms -
equals expected_view on every small case at every pass length, while each deliberately wrong restatement (no carry, the
last word read past its end, no r == 0 arm, the total arm replaced by the last word's base, a rank counted with <=, a kNN
mask that lets ids >= n_docs through) disagrees with it on a named case: the inputs can see that class of bug."""
import functools

import numpy as np
import pytest

import filter_cases as FC
from test_gpu_filter import FilteredDesc

PASS_LENGTHS = (1, 2, 3, FC.PASS_TILES)


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, host index, host base with a made-up post_ref and graph, allowed sets) of a small case; nothing is uploaded."""
    case = FC.make(name)
    ix = case.build()
    n_docs = case.n_docs
    rng = np.random.default_rng(len(name))
    graph = rng.integers(0, n_docs, 3 * n_docs).astype(np.uint32)
    graph[::7] = n_docs + rng.integers(0, 5, len(graph[::7]))      # ids the API refuses: the d < n_docs arm
    graph[3::11] = 0xffffffff
    base = FC.host_base(ix.desc, graph)
    return case, ix, base, FC.allowed_sets(ix.desc, base["post_doc"])


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_case_has_its_properties_and_its_sets_their_shape(name):
    case, ix, base, sets = _built(name)
    found = case.check(ix.desc)
    kept = FC.check_sets(sets, base["post_doc"], single=case.single)
    print("filter case %s: %s -> %s; kept postings per set: %s" % (name, case.paths, found, kept))
    if int(ix.desc.n_postings):
        assert {"first", "last", "lane0", "lane63", "lanes31_32", "words_even", "tiles_even", "tiles_odd", "all_but_one"} <= set(sets)
        assert kept["first"] == kept["last"] == 1 and kept["all_but_one"] == int(ix.desc.n_postings) - 1
    assert sets["doc_ids"][0].sum() == 4


def test_the_big_case_has_its_properties():
    """check() of the 8 400 037-posting case on the host build (the GPU test builds the same collection device-assisted)."""
    case = FC.make("big")
    ix = case.build()
    print("filter case big: %s -> %s" % (case.paths, case.check(ix.desc)))
    post_doc = FC.host_base(ix.desc)["post_doc"]
    sets = FC.allowed_sets(ix.desc, post_doc, names=FC.BIG_SETS)
    assert set(sets) == set(FC.BIG_SETS)
    FC.check_sets(sets, post_doc)
    print("kept postings before / from tile 4096:", FC.check_big_sets(sets, post_doc))


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_expected_view_agrees_with_filtered_desc(name):
    case, ix, base, sets = _built(name)
    for sname, (allowed, _) in sets.items():
        want = FC.expected_view(base, allowed, case.n_docs)
        fd = FilteredDesc(ix.desc, allowed)
        assert np.array_equal(want["block_post_start"].astype(np.uint64), fd.bps), sname
        assert np.array_equal(want["post_doc"], fd.post_doc) and int(fd.desc.n_postings) == len(want["post_doc"]), sname
        assert len(want["block_post_start"]) == int(ix.desc.n_blocks) + 1
        # what the reference says beyond FilteredDesc, from the definition: one ref per kept posting, still its document's
        assert np.array_equal(want["post_ref"], base["post_ref"][allowed[base["post_doc"]]])
        assert want["count"] == int(allowed.sum()) and len(want["bits"]) == -(-case.n_docs // 32)
        bits = np.unpackbits(want["bits"].view(np.uint8), bitorder="little")
        assert np.array_equal(bits[:case.n_docs].astype(bool), allowed) and not bits[case.n_docs:].any()
        g = base["knn"]
        assert np.array_equal(want["knn"] != FC.NONE, (g < case.n_docs) & allowed[np.minimum(g, case.n_docs - 1)])


@pytest.mark.parametrize("name", FC.CASE_NAMES)
def test_the_restated_device_algorithm_equals_expected_view(name):
    case, ix, base, sets = _built(name)
    for sname, (allowed, _) in sets.items():
        want = FC.expected_view(base, allowed, case.n_docs)
        for pass_tiles in PASS_LENGTHS:
            diff = FC.view_diff(FC.device_view(base, allowed, case.n_docs, pass_tiles), want)
            assert diff is None, (sname, pass_tiles, diff)


def _seen(wrong, name, pass_tiles=FC.PASS_TILES):
    """The allowed sets of the case on which the wrong restatement's view is not the expected one."""
    case, ix, base, sets = _built(name)
    out = []
    for sname, (allowed, _) in sets.items():
        want = FC.expected_view(base, allowed, case.n_docs)
        assert FC.view_diff(FC.device_view(base, allowed, case.n_docs, pass_tiles), want) is None
        if FC.view_diff(FC.device_view(base, allowed, case.n_docs, pass_tiles, wrong=wrong), want) is not None:
            out.append(sname)
    return out


def test_a_scan_without_the_carry_is_seen():
    # 5000 postings are three tiles: passes of one or two tiles hand a carry over, the shipped pass length does not
    for pass_tiles in (1, 2):
        seen = _seen("no_carry", "exact_5000", pass_tiles)
        assert {"all", "first", "lane0", "lane63", "tiles_even", "all_but_one", "p50"} <= set(seen), seen
        assert "none" not in seen and "last" not in seen      # (nothing kept before the last pass: no carry to lose)
    assert _seen("no_carry", "exact_5000") == []
    assert "all" in _seen("no_carry", "exact_2049", 1) and _seen("no_carry", "exact_2048", 1) == []   # two tiles; one


def test_a_last_word_read_past_its_end_is_seen():
    for P in (1, 63, 65, 2047, 2049, 5000):
        seen = _seen("past_end", "exact_%d" % P)
        assert {"all", "none", "first", "last"} <= set(seen), (P, seen)
    for P in (0, 64, 2048, 4096):                    # whole words (or none): there is no such lane
        assert _seen("past_end", "exact_%d" % P) == [], P
    assert _seen("past_end", "blocks") == []


def test_a_block_remap_without_the_r0_arm_is_seen():
    seen = _seen("no_r0_arm", "blocks")
    assert {"all", "lane0", "words_even", "p50", "holes"} <= set(seen), seen
    assert "none" not in seen


def test_a_total_arm_that_takes_the_last_words_base_is_seen():
    seen = _seen("total_is_last_base", "blocks")     # n_postings = 40 whole words: the last start is past the last word
    assert {"all", "last", "lane63", "all_but_one", "p50", "holes"} <= set(seen), seen
    assert "none" not in seen
    for P in (64, 2048, 4096):
        assert "all" in _seen("total_is_last_base", "exact_%d" % P), P
    for P in (63, 65, 5000):                         # the last start lies inside the last word: the arm is not taken
        assert _seen("total_is_last_base", "exact_%d" % P) == [], P


def test_a_rank_counted_with_le_is_seen():
    for name in ("exact_1", "exact_64", "exact_5000", "blocks"):
        seen = _seen("rank_le", name)
        assert {"all", "first", "last"} <= set(seen), (name, seen)
        assert "none" not in seen


def test_a_knn_mask_that_lets_foreign_ids_through_is_seen():
    for name in ("exact_0", "exact_65", "blocks"):
        case, ix, base, sets = _built(name)
        assert (base["knn"] >= case.n_docs).any()
        assert set(_seen("knn_oob", name)) == set(sets), name
