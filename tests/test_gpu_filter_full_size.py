"""Document filters at full size: the 8.8M-document bench collection with the bench parameters, a random 10 % filter,
256 queries at k = 10. Approximate search equals the oracle on I_A; device filtered exact equals host filtered exact.
Run with `-m gpu`."""
import numpy as np
import pytest

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from test_gpu_filter import FilteredDesc, _same

pytestmark = pytest.mark.gpu


def test_bench_collection_10_percent_filter_256_queries():
    dim, n_docs, nq = 30_000, 8_800_000, 256
    docs = _native.synth(n_docs, dim, 42, 0)
    ix = _native.NativeIndex.build(2, dim, *docs, BuildConfig.defaults(n_postings=2000, centroid_fraction=0.2,
                                                                        summary_energy=0.5, max_fraction=6.0, use_device=1))
    ix.upload(0)
    q = _native.synth(nq, dim, 43, 1, docs)
    del docs
    allowed = np.random.default_rng(7).random(n_docs) < 0.10
    f = ix.make_filter(allowed)
    g = ix.batch_search(*q, 10, 4, 1.0, False, filter=f)
    fd = FilteredDesc(ix.desc, allowed)   # (holds the arrays its descriptor points to)
    _same(g, orc.batch_search(fd.desc, *q, 10, 4, 1.0, False)[:3])
    assert (g[2] > 0).all()
    d = ix.exact_search_device(*q, 10, filter=f)
    h = ix.exact_search(*q, 10, filter=f)
    assert (d[2] == 10).all()
    _same(d, h)
