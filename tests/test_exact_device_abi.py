"""sgpu_exact_search_device without a GPU: the entry point is exported and declared, and its argument checks come
before the device check (an index that was built but never uploaded)."""
import ctypes
import os
import re

import numpy as np

import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGPU_EINVAL, SGPU_EDEVICE, SGPU_ELIMIT = 1, 2, 5


def test_exact_search_device_is_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    assert re.search(r"\bsgpu_exact_search_device\s*\(", hdr)
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sgpu_exact_search_device")
    assert _native.lib().sgpu_abi_version() == 4


def _call(ix, q_off, comps, vals, k):
    L = _native.lib()
    q_off = np.ascontiguousarray(q_off, np.uint64)
    comps = np.ascontiguousarray(comps, np.uint32)
    vals = np.ascontiguousarray(vals, np.float32)
    nq = len(q_off) - 1
    sc = np.zeros((nq, max(k, 1)), np.float32)
    ids = np.zeros((nq, max(k, 1)), np.uint64)
    n = np.zeros(max(nq, 1), np.uint32)
    p = _native._p
    st = L.sgpu_exact_search_device(ix.h, 0, p(q_off), p(comps), p(vals), nq, k, p(sc), p(ids), p(n))
    return st, L.sgpu_last_error().decode()


def test_argument_checks_before_the_device_check():
    dim = 300
    off, comps, vals = random_dataset(11, 200, dim)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    good = ([0, 2], [1, 5], [1.0, 2.0])
    st, msg = _call(ix, *good, 0)
    assert st == SGPU_EINVAL and "k" in msg
    st, msg = _call(ix, *good, 1025)
    assert st == SGPU_ELIMIT and "1024" in msg
    st, msg = _call(ix, [0, 2], [5, 1], [1.0, 2.0], 10)          # components not ascending
    assert st == SGPU_EINVAL and msg
    st, msg = _call(ix, [0, 1], [dim], [1.0], 10)                # component out of range
    assert st == SGPU_EINVAL and msg
    st, msg = _call(ix, *good, 10)                               # valid, but the index is on no device
    assert st == SGPU_EDEVICE and "upload" in msg
    st, msg = _call(ix, *good, 1024)
    assert st == SGPU_EDEVICE


def test_dataset_batch_search_host_path_unchanged():
    ds = seismic_amd.SeismicDataset()
    ds.add_document("d0", ["x", "y"], [1.0, 2.0])
    ds.add_document("d1", ["y", "z"], [4.0, 5.0])
    ds.add_document("d2", [], [])
    qs = [np.array(["y", "nope"], dtype="U30"), np.array(["z"], dtype="U30"), np.array([], dtype="U30")]
    vs = [np.array([2.0, 1.0], np.float32), np.array([-1.0], np.float32), np.array([], np.float32)]
    want = [[("a", 8.0, "d1"), ("a", 4.0, "d0")], [("b", 0.0, "d0"), ("b", 0.0, "d2")],
            [("c", 0.0, "d0"), ("c", 0.0, "d1")]]
    assert ds.batch_search(["a", "b", "c"], qs, vs, 2) == want
    assert ds.batch_search(["a", "b", "c"], qs, vs, 2, device=None) == want
    assert [ds.search(q, c, v, 2) for q, c, v in zip("abc", qs, vs)] == want
