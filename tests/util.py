"""Shared helpers for the tests (seeded small datasets, index comparison)."""
import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig


def random_dataset(seed, n_docs, dim, nnz_lo=4, nnz_hi=40, empty_every=0, value_scale=1.0):
    rng = np.random.default_rng(seed)
    vecs = []
    for d in range(n_docs):
        if empty_every and d % empty_every == empty_every - 1:
            vecs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        n = int(rng.integers(nnz_lo, nnz_hi + 1))
        c = np.sort(rng.choice(dim, min(n, dim), replace=False)).astype(np.uint32)
        v = (rng.exponential(0.45, len(c)) * value_scale + 0.02).astype(np.float32)
        vecs.append((c, v))
    return orc.csr(vecs)


def random_queries(seed, nq, dim, nnz_lo=3, nnz_hi=30):
    rng = np.random.default_rng(seed)
    vecs = []
    for _ in range(nq):
        n = int(rng.integers(nnz_lo, nnz_hi + 1))
        c = np.sort(rng.choice(dim, min(n, dim), replace=False)).astype(np.uint32)
        v = (rng.exponential(0.45, len(c)) + 0.02).astype(np.float32)
        v = v + np.arange(len(c), dtype=np.float32) * 1e-4   # distinct weights
        vecs.append((c, v))
    return orc.csr(vecs)


_SCALARS = ("comp_width", "n_docs", "dim", "nnz", "n_blocks", "n_postings", "n_rows", "n_entries")
# arrays whose elements belong to one block (desc_diff names it and its postings)
_BLOCK_LEVEL = ("block_post_start", "blk_min", "blk_quant", "post_doc")


def _owner(starts, i):
    """Index of the range [starts[j], starts[j+1]) that holds i (the last one that starts at or before it)."""
    return int(np.searchsorted(np.asarray(starts).astype(np.int64), i, side="right") - 1)


def desc_diff(a, b):
    """None where the two descriptors are bit-identical; otherwise a sentence naming the first differing array (in the
    descriptor's order), the list the element belongs to and, for block-level arrays, the global block, its posting
    range and the two values."""
    for f in _SCALARS:
        if getattr(a, f) != getattr(b, f):
            return "%s: %d != %d" % (f, getattr(a, f), getattr(b, f))
    A, B = orc.desc_arrays(a), orc.desc_arrays(b)
    for k in A:
        x, y = A[k], B[k]
        if x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            continue
        if x.shape != y.shape:
            return "%s: %d != %d elements" % (k, len(x), len(y))
        xb, yb = x.view("u%d" % x.dtype.itemsize), y.view("u%d" % y.dtype.itemsize)
        i = int(np.flatnonzero(xb != yb)[0])
        what = "%s[%d]: %r (0x%x) != %r (0x%x)" % (k, i, x[i].item(), int(xb[i]), y[i].item(), int(yb[i]))
        lbs, bps = A["list_block_start"], A["block_post_start"]
        if k in ("fwd_offsets", "list_block_start", "list_row_start"):
            return what + (" (document %d)" % i if k == "fwd_offsets" else " (list %d)" % min(i, a.dim - 1))
        if k in ("fwd_comps", "fwd_vals"):
            return what + " (document %d)" % _owner(A["fwd_offsets"], i)
        if k in _BLOCK_LEVEL:
            blk = _owner(bps, i) if k == "post_doc" else min(i, a.n_blocks - 1)
            return what + " (list %d, block %d = its block %d, postings [%d, %d) of a: %s; of b: %s)" % (
                _owner(lbs, blk), blk, blk - int(lbs[_owner(lbs, blk)]), bps[blk], bps[blk + 1],
                A["post_doc"][int(bps[blk]): int(bps[blk + 1])][:12].tolist(),
                B["post_doc"][int(B["block_post_start"][blk]): int(B["block_post_start"][blk + 1])][:12].tolist())
        row = _owner(A["row_ptr"], i) if k in ("sum_bid", "sum_code") else min(i, a.n_rows - 1)
        lst = _owner(A["list_row_start"], row)
        what += " (list %d, row %d = component %d" % (lst, row, A["row_comp"][row])
        if k in ("sum_bid", "sum_code"):
            blk = int(lbs[lst]) + int(A["sum_bid"][i])
            what += ", a's block %d: postings [%d, %d), blk_min %r, blk_quant %r" % (
                blk, bps[blk], bps[blk + 1], A["blk_min"][blk].item(), A["blk_quant"][blk].item())
        return what + ")"
    return None


def desc_equal(a, b):
    diff = desc_diff(a, b)
    assert diff is None, diff


def row_dir_bucket(key, n_buckets):
    """device_types.hpp: row_dir_bucket restated - hash, then multiply-high onto [0, n_buckets)."""
    return (((int(key) * 2654435761) & 0xffffffff) * int(n_buckets)) >> 32


def row_dir_table(ix):
    """The hashed row directory as uploaded (sgpu_debug_row_dir): (table [bucket][slot][word] u32, buckets); buckets == 0
    where the index has none (u32 components)."""
    import ctypes
    L = _native.lib()
    L.sgpu_debug_row_dir.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    nw, nbk = ctypes.c_uint64(0), ctypes.c_uint32(0)
    assert L.sgpu_debug_row_dir(ix.h, None, 0, ctypes.byref(nw), ctypes.byref(nbk)) == 0
    if nbk.value == 0:
        return np.zeros((0, 4, 4), np.uint32), 0
    assert nw.value == 16 * nbk.value
    tab = np.zeros(nw.value, np.uint32)
    assert L.sgpu_debug_row_dir(ix.h, tab.ctypes.data_as(ctypes.c_void_p), nw.value, ctypes.byref(nw), ctypes.byref(nbk)) == 0
    return tab.reshape(-1, 4, 4), nbk.value


def row_dir_lookup(tab, n_buckets, key):
    """The kernel's walk (search_stage01.inc: build_row_table) restated: (entry words, bucket it was found in) of `key`, or
    (None, bucket whose empty slot ended the walk)."""
    b = row_dir_bucket(key, n_buckets)
    for _ in range(n_buckets + 1):
        keys = tab[b, :, 0]
        hit = np.nonzero(keys == key)[0]
        if len(hit):
            return tab[b, hit[0]], b
        if np.any(keys == 0xffffffff):
            return None, b
        b = 0 if b + 1 == n_buckets else b + 1
    raise AssertionError("probe sequence does not end")
