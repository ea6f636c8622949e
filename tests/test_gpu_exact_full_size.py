"""Device exact search at full size: the 8.8M-document bench collection, 256 queries at k = 10, bit-identical to the
host exact search. Run with `-m gpu`."""
import numpy as np
import pytest

from seismic_amd import _native
from seismic_amd._abi import BuildConfig

pytestmark = pytest.mark.gpu


def test_bench_collection_256_queries_bit_identical():
    dim, n_docs, nq = 30_000, 8_800_000, 256
    docs = _native.synth(n_docs, dim, 42, 0)
    ix = _native.NativeIndex.build(2, dim, *docs, BuildConfig.defaults(n_postings=1, centroid_fraction=1.0,
                                                                        min_cluster_size=0, summary_energy=1.0,
                                                                        max_fraction=1.0, doc_cut=1))
    ix.upload(0)
    q = _native.synth(nq, dim, 43, 1, docs)
    del docs
    ds, di, dn = ix.exact_search_device(*q, 10)
    hs, hi, hn = ix.exact_search(*q, 10)
    assert (dn == 10).all() and np.array_equal(dn, hn)
    assert np.array_equal(di, hi)
    assert np.array_equal(ds.view(np.uint32), hs.view(np.uint32))
