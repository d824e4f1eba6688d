"""shared helpers for the parity tests."""
import glob
import os
import numpy as np
from conftest import MTX


def all_fixture_mtx(include_pattern=False):
    files = sorted(glob.glob(os.path.join(MTX, "*", "*.mtx")))
    if not include_pattern:
        files = [f for f in files if "pattern" not in f and "complex" not in f]
    return files


def dok_from_coo(rows, cols, vals):
    d = {}
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        d[(r, c)] = d.get((r, c), 0.0) + v
    return d


def scipy_csr(num_rows, num_cols, rows, cols, vals, dtype=np.float64):
    import scipy.sparse as sp
    return sp.coo_matrix((np.asarray(vals, dtype=dtype), (rows, cols)), shape=(num_rows, num_cols)).tocsr()


def bmsp_host_to_dok(num_rows, num_cols, keys, bmps, offsets, values, transposed=False):
    """expand the four bmSparse arrays to {(r,c): v} straight from the format definition."""
    out = {}
    for b in range(len(keys)):
        brow, bcol = int(keys[b]) >> 32, int(keys[b]) & 0xFFFFFFFF
        bmp, off, k = int(bmps[b]), int(offsets[b]), 0
        for p in range(64):
            if bmp >> (63 - p) & 1:
                hi, lo = p // 8, p % 8
                r, c = (brow * 8 + lo, bcol * 8 + hi) if transposed else (brow * 8 + hi, bcol * 8 + lo)
                out[(r, c)] = float(values[off + k])
                k += 1
    return out


def assert_bmsp_equal_exact(oracle_m, keys, bmps, offsets, values, np_dtype):
    """bit-exact comparison of the product's four arrays with the oracle's matrix."""
    nb = oracle_m.block_num
    assert len(keys) == nb, (len(keys), nb)
    np.testing.assert_array_equal(np.asarray(keys, dtype=np.uint64), oracle_m.keys)
    np.testing.assert_array_equal(np.asarray(bmps, dtype=np.uint64)[:nb], oracle_m.bmps)
    np.testing.assert_array_equal(np.asarray(offsets, dtype=np.uint64)[:nb + 1], oracle_m.offsets)
    ref = oracle_m.values.astype(np_dtype)
    got = np.asarray(values)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))


# every kernel bmsp_spmv can be made to launch on the gap matrices of test_spgemm_special_values._gap_matrix
SPMV_LAUNCHES = {
    # name -> (matrix kind, environment, variant, kernel name prefix)
    "vstream_cached_atomic": ("sparse", {"BMSP_SPMV_NOCHUNK": "1", "BMSP_SPMV_RED": "0"}, 0, "spmv_vstream_kernel<kCached, kAtomic>"),
    "vstream_cached_sorted": ("sparse", {"BMSP_SPMV_NOCHUNK": "1", "BMSP_SPMV_RED": "1"}, 0, "spmv_vstream_kernel<kCached, kSorted>"),
    "vstream_decode_atomic": ("sparse", {"BMSP_SPMV_NO_POSCACHE": "1", "BMSP_SPMV_RED": "0"}, 0, "spmv_vstream_kernel<kDecode, kAtomic>"),
    "vstream_decode_sorted": ("sparse", {"BMSP_SPMV_NO_POSCACHE": "1", "BMSP_SPMV_RED": "1"}, 0, "spmv_vstream_kernel<kDecode, kSorted>"),
    "rowgroup": ("dense", {}, 3, "spmv_rowgroup_kernel"),
    "rowgroup_sparse": ("sparse", {}, 3, "spmv_rowgroup_kernel"),
    "blockrow_batched": ("dense", {}, 1, "spmv_blockrow_kernel<64"),
    "blockrow_batched_sparse": ("sparse", {}, 1, "spmv_blockrow_kernel<64"),
    "blockrow_8": ("sparse", {}, 2, "spmv_blockrow_kernel<8"),
    "sweep_round1": ("sparse", {"BMSP_SPMV_OLD": "1"}, 0, "spmv_sweep_kernel"),
    "sweep_round1_full": ("dense", {"BMSP_SPMV_NO_ROWGROUP": "1"}, 0, "spmv_sweep_kernel<FULL>"),
    # the chunked sweep, forced (the default takes it from a few thousand chunks only): row-sorted words and the storage-order words
    "chunk_row_sorted": ("sparse", {"BMSP_SPMV_CHUNK": "1"}, 0, "spmv_chunk_kernel"),
    "chunk_storage_order": ("sparse", {"BMSP_SPMV_CHUNK": "1", "BMSP_SPMV_CHUNK_SORTED": "0"}, 0, "spmv_chunk_kernel"),
}
# launches that exist for some dtypes only (the chunked sweep is an fp32 kernel), and what bmsp_spmv_chunk_layout must report for them
SPMV_LAUNCH_DTYPES = {"chunk_row_sorted": (0,), "chunk_storage_order": (0,)}
SPMV_CHUNK_LAYOUT = {"chunk_row_sorted": 2, "chunk_storage_order": 1}


def spmv_launch_params(dtypes=(0, 1, 2)):
    """(launch, dtype) for every entry of SPMV_LAUNCHES and every dtype its kernel exists for"""
    return [(l, d) for l in SPMV_LAUNCHES for d in dtypes if d in SPMV_LAUNCH_DTYPES.get(l, (0, 1, 2))]


# every SpMM kernel test_spmm.py pins, on the same two matrix kinds (spmm_kernel<64> needs 2^32 values and is out of reach)
SPMM_LAUNCHES = {
    # name -> (matrix kind, BMSP_SPMM_NO_VSTREAM, k, kernel)
    "vstream4": ("sparse", False, 3, "spmm_vstream_kernel<4>"),
    "vstream8": ("sparse", False, 7, "spmm_vstream_kernel<8>"),
    "kernel4": ("sparse", True, 3, "spmm_kernel<4>"),
    "kernel16": ("sparse", True, 13, "spmm_kernel<16>"),
    "wide": ("sparse", True, 21, "spmm_wide_kernel"),
    "kernel4_dense": ("dense", False, 4, "spmm_kernel<4>"),
    "kernel16_dense": ("dense", False, 9, "spmm_kernel<16>"),
    "wide_dense": ("dense", False, 33, "spmm_wide_kernel"),
}
