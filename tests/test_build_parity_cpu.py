"""Oracle builder vs host builder on signed, tied and edge values and at the structural edges of the build
(tests/build_cases.py): byte-identical descriptors, single-threaded and on all cores, and every case's predicate -
the proof that the case reaches the edge it is named after. No GPU; test_gpu_build_parity.py runs the same cases
through the device-assisted build."""
import numpy as np
import pytest

import build_cases as BC
import orc
from seismic_amd import _native
from util import desc_diff, desc_equal


@pytest.mark.parametrize("name", BC.NAMES)
def test_host_builder_matches_oracle_and_case_reaches_its_edge(name):
    case = BC.get(name)
    want = orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config())
    case.check(orc.desc_arrays(want.desc))
    for nt in (1, 0):
        built = _native.NativeIndex.build(case.cw, case.dim, *case.docs, case.build_config(num_threads=nt))
        desc_equal(want.desc, built.desc)


def test_case_names_cover_the_laws_and_the_entry_counts():
    assert {"law_" + law for law in BC.LAWS} <= set(BC.NAMES)
    assert BC.ENTRY_COUNTS == (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
    assert BC.NC_WANTED == (1, 63, 64, 65, 128, 129)


def test_zero_inputs_become_signed_zeros():
    assert BC.f16_bits(BC.ZEROS).tolist() == [0x0000, 0x0000, 0x8000, 0x8000, 0x0000]


def test_desc_diff_names_the_place():
    case = BC.get("law_signed_ties")
    a = orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config())
    b = orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config())
    assert desc_diff(a.desc, b.desc) is None
    A, B = orc.desc_arrays(a.desc), orc.desc_arrays(b.desc)
    lst = int(np.flatnonzero(BC.list_blocks(A) > 1)[0])
    blk = int(A["list_block_start"][lst]) + 1
    p0, p1 = int(A["block_post_start"][blk]), int(A["block_post_start"][blk + 1])
    B["blk_min"][blk] = -B["blk_min"][blk] if B["blk_min"][blk] != 0 else np.float32(-0.0)   # (views: writes b's arrays)
    msg = desc_diff(a.desc, b.desc)
    assert msg.startswith("blk_min[%d]" % blk) and "list %d, block %d" % (lst, blk) in msg
    assert "postings [%d, %d)" % (p0, p1) in msg and repr(A["blk_min"][blk].item()) in msg
    with pytest.raises(AssertionError, match="blk_min"):
        desc_equal(a.desc, b.desc)
    B["post_doc"][p0], B["post_doc"][p0 + 1] = B["post_doc"][p0 + 1], B["post_doc"][p0]      # an earlier array wins
    msg = desc_diff(a.desc, b.desc)
    assert msg.startswith("post_doc[%d]" % p0) and "list %d, block %d" % (lst, blk) in msg
    c = orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config(summary_energy=0.9))
    assert desc_diff(a.desc, c.desc).startswith("n_rows")
