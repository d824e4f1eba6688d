"""Fold cases of the chunked SpMV sweep (spmv_chunk_kernel): chunks with a head slot, a tail slot, both and neither, folds over two, three
and more chunks, hub chunks beside window chunks, the partial last chunk.  The matrices are laid out block-row by block-row so that the
512-value chunks fall where each case needs them; every case runs with BMSP_SPMV_CHUNK=1, NaN-poisoned y, bitwise equality across
sweeps, and the oracle within check_spmv's bound."""
import numpy as np
import pytest
import util

pytestmark = pytest.mark.gpu

V = 512  # stored values per chunk (kChV)


@pytest.fixture
def force_chunks(monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")


def layout(counts, seed):
    """counts: {block-row: stored values}, one value per tile (distinct block columns), rows spread over the block-row's 8 rows"""
    g = np.random.default_rng(seed)
    cells = []
    for br, k in counts.items():
        bcs = np.sort(g.choice(4096, k, replace=False))
        cells += [(8 * br + int(g.integers(0, 8)), 8 * int(bc) + int(g.integers(0, 8))) for bc in bcs]
    return np.asarray(cells, dtype=np.int64)


def chunks_of(counts):
    """per chunk: (head, tail, one block-row only) as build_chunk_cache sets them"""
    brs = np.repeat(list(counts.keys()), list(counts.values()))
    nch = (brs.size + V - 1) // V
    fb = [int(brs[c * V]) for c in range(nch)]
    lb = [int(brs[min((c + 1) * V, brs.size) - 1]) for c in range(nch)]
    out = []
    for c in range(nch):
        head = c > 0 and lb[c - 1] == fb[c]
        tail = c + 1 < nch and fb[c + 1] == lb[c] and not (head and fb[c] == lb[c])
        out.append((head, tail, fb[c] == lb[c]))
    return out


def run(oracle, bmsp, nr, nc, cells, seed, sweeps=3):
    from pybmsp import gen
    cells = np.unique(cells, axis=0)
    r, c = cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32)
    v = np.random.default_rng(seed).uniform(0.1, 1.0, len(cells))
    A = bmsp.BmSpMatrix.from_coo(nr, nc, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"] == "spmv_chunk_kernel"
    x = gen.spmv_x(nc, "cusp")
    dx = bmsp.DeviceArray.from_host(x)
    ys = []
    for _ in range(sweeps):
        y = bmsp.DeviceArray(nr, np.float32)
        assert bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * 4) == 0  # NaN poison: every row must be written
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, dx.ptr, y.ptr, 0, None))
        ys.append(y.to_host())
    assert np.all(np.isfinite(ys[0]))
    for yk in ys[1:]:
        np.testing.assert_array_equal(ys[0].view(np.uint8), yk.view(np.uint8))
    y_ref = oracle.spmv_f32(oracle.bmsp_from_coo(oracle.Coo(nr, nc, r, c, v), 0, False), x)
    S = util.scipy_csr(nr, nc, r, c, np.asarray(v, np.float32).astype(np.float64))
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    assert np.all(np.abs(ys[0] - y_ref) <= bound + 1e-5 * np.abs(y_ref)), np.max(np.abs(ys[0] - y_ref))


# block-row -> values.  Cuts at multiples of 512:
#   br 1 crosses 512 (two-way fold: chunk 0 tail, chunk 1 head); br 4 spans chunks 1 .. 4 (four-way; chunks 2 and 3 hold br 4 alone);
#   chunk 4 folds br 4 as a head and br 6 as a tail (two folds, their last arrivers may differ); chunk 5 ends exactly on br 10;
#   chunk 6 is br 11 alone with no fold; chunk 7 has neither head nor tail; chunk 8 is br 14 alone, a tail only; chunk 9 is a head (br 14)
#   and a tail (br 15, three-way over chunks 9 .. 11); chunk 11 is the partial last chunk; block-rows 3, 7, 8 and 17 .. 31 are empty
LAYOUT = {0: 300, 1: 400, 2: 100, 4: 1500, 5: 200, 6: 100, 9: 400, 10: 72, 11: 512, 12: 100, 13: 412, 14: 600, 15: 1000, 16: 30}


def test_layout_has_every_case():
    ch = chunks_of(LAYOUT)
    assert len(ch) == 12 and sum(LAYOUT.values()) % V != 0
    assert ch[0] == (False, True, False)      # tail only
    assert ch[1] == (True, True, False)       # both
    assert ch[2] == (True, False, True)       # one block-row, head
    assert ch[4] == (True, True, False)       # both, two different folds
    assert ch[5] == (True, False, False)      # head only, ends on a block-row
    assert ch[6] == (False, False, True)      # one block-row, no fold
    assert ch[7] == (False, False, False)     # neither
    assert ch[8] == (False, True, True)       # one block-row, tail
    assert ch[9] == (True, True, False)


def test_fold_layout(oracle, bmsp, force_chunks):
    run(oracle, bmsp, 256, 4096 * 8, layout(LAYOUT, 11), 11)


@pytest.mark.parametrize("shift", [1, 7, 100, 255, 256, 511])
def test_fold_layout_shifted(oracle, bmsp, force_chunks, shift):
    # the same block-rows behind `shift` values in block-row 0: every cut moves, folds change width and partner
    counts = dict(LAYOUT)
    counts[0] += shift
    run(oracle, bmsp, 256, 4096 * 8, layout(counts, shift), shift)


def test_many_short_folds(oracle, bmsp, force_chunks):
    # block-rows of 400 .. 1200 values: nearly every chunk a head and a tail, folds of two and three chunks, under a few hundred waves
    g = np.random.default_rng(21)
    counts = {br: int(g.integers(400, 1200)) for br in range(300)}
    ch = chunks_of(counts)
    assert sum(h and t for h, t, _ in ch) > len(ch) // 3
    run(oracle, bmsp, 8 * 300 + 5, 4096 * 8, layout(counts, 21), 21)


def test_hub_row_between_sparse_rows(oracle, bmsp, force_chunks):
    # one hub block-row of 40 chunks between block-rows of a few values: its slots are written by hub chunks and by window chunks
    g = np.random.default_rng(22)
    counts = {br: int(g.integers(1, 40)) for br in range(100)}
    counts[50] = 40 * V + 123
    cells = layout({k: v for k, v in counts.items() if v <= 4096}, 22)
    bc = np.arange(counts[50])
    hub = np.stack([8 * 50 + g.integers(0, 8, bc.size), bc * 3 + g.integers(0, 3, bc.size)], axis=1)
    run(oracle, bmsp, 800, 3 * counts[50] + 8, np.concatenate([cells, hub]), 22)
