"""Device-assisted build (build_assign.hip, build_summaries.hip) vs the host builder and, for the small cases, the
oracle's builder, on the cases of tests/build_cases.py: signed, tied, zero and binary16-edge values, 1 / 63..129 / len
centroids per list, every cluster dissolved, 1..4097 document entries per block. Bit equality, nothing else.
test_build_parity_cpu.py proves that every case reaches its edge. Run with `-m gpu`."""
import numpy as np
import pytest

import build_cases as BC
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import desc_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", BC.NAMES)
def test_device_build_matches_host_and_oracle(name):
    case = BC.get(name)
    host = _native.NativeIndex.build(case.cw, case.dim, *case.docs, case.build_config())
    dev = _native.NativeIndex.build(case.cw, case.dim, *case.docs, case.build_config(use_device=1))
    desc_equal(host.desc, dev.desc)
    if case.n_docs < 2000:
        want = orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config())
        desc_equal(want.desc, dev.desc)
    if name in BC.ZEROS_CASES:   # how many blocks the -0.0 rule leaves to the host summariser (run with -s)
        A = orc.desc_arrays(dev.desc)
        neg = np.zeros(case.n_docs, bool)
        doc_of = np.repeat(np.arange(case.n_docs), np.diff(case.docs[0].astype(np.int64)))
        neg[doc_of[BC.f16_bits(case.docs[2]) == 0x8000]] = True
        first = A["block_post_start"][:-1].astype(np.int64)
        routed = np.add.reduceat(neg[A["post_doc"].astype(np.int64)].astype(np.int64), first) > 0
        print("build parity: %s: %d of %d blocks hold a -0.0 value and are summarised on the host" % (
            name, int(routed.sum()), len(routed)))
        assert routed.any()


def test_both_assignment_routes_in_one_build_with_signed_ties():
    """The dim-64 configuration of test_gpu_build.py at its size, with values whose approximate dots cancel to +0.0
    and tie. Component 0 is in 87 % of the documents: its list has more centroids than the assignment kernel takes
    (device_assign_max_centroids: 8192 on gfx950) and is clustered on the host inside the device build. Component 32
    is in 60 %: ~6000 centroids, the device's route near its limit. The other lists have some 900 (short documents keep
    the host build, which is most of this test, to a few seconds)."""
    dim, n_docs = 64, 40_000
    rng = np.random.default_rng(111)
    docs = []
    for d in range(n_docs):
        if d % 53 == 52:
            docs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        c = rng.choice(dim, int(rng.integers(3, 9)), replace=False)
        c = c[(c != 0) & (c != 32)]
        c = np.r_[c, [0] * (rng.random() < 0.87), [32] * (rng.random() < 0.60)]
        c = np.sort(c).astype(np.uint32)
        docs.append((c, BC.LAWS["signed_ties"](rng, len(c))))
    D = orc.csr(docs)
    cfg = dict(n_postings=20000, centroid_fraction=0.257, summary_energy=0.4, max_fraction=6.0, min_cluster_size=0)
    host = _native.NativeIndex.build(2, dim, *D, BuildConfig.defaults(**cfg))
    dev = _native.NativeIndex.build(2, dim, *D, BuildConfig.defaults(use_device=1, **cfg))
    desc_equal(host.desc, dev.desc)
    nc = BC.centroids_of(BC.list_lengths(orc.desc_arrays(host.desc)), 0.257)
    assert nc[0] > 8192 and 4096 < nc[32] <= 8192 and 64 < np.delete(nc, [0, 32]).max() < 2048, nc
