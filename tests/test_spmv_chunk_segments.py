"""Segment cases of the chunked SpMV sweep's reduction by block-row (spmv_chunk_kernel, chunk_seg_reduce): lane l of a chunk holds its
values 8l .. 8l+7, and a block-row may end on a lane boundary, lie inside one lane beside others, run across every lane of a chunk, or
be absent from the window.  Each matrix is laid out block-row by block-row so that the 512-value chunks and the 8-value lanes fall where
the case needs them; every case runs with BMSP_SPMV_CHUNK=1, NaN-poisoned y, bitwise equality across sweeps, and the oracle within
check_spmv's bound."""
import numpy as np
import pytest
import util

V = 512    # stored values per chunk (kChV)
PER = 8    # ... per lane
NC = 4096 * 8


@pytest.fixture
def force_chunks(monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")


def layout(counts, seed):
    """counts: [(block-row, stored values)] in increasing block-row order; the values of a block-row are distinct cells of its 8 rows"""
    g = np.random.default_rng(seed)
    cells = []
    for br, k in counts:
        idx = g.choice(8 * NC, k, replace=False)
        cells.append(np.stack([8 * br + idx // NC, idx % NC], axis=1))
    return np.concatenate(cells).astype(np.int64)


def lanes(counts):
    """per (chunk, lane): the block-rows of the lane's values, in storage order (the partial last chunk's empty lanes left out)"""
    brs = np.repeat([b for b, _ in counts], [k for _, k in counts])
    return {(i // V, (i % V) // PER): brs[i:i + PER] for i in range(0, brs.size, PER)}


def windows(counts):
    brs = np.repeat([b for b, _ in counts], [k for _, k in counts])
    return [int(brs[min(c + V, brs.size) - 1] - brs[c] + 1) for c in range(0, brs.size, V)]


def run(oracle, bmsp, counts, seed, sweeps=3):
    from pybmsp import gen
    cells = layout(counts, seed)
    assert max(windows(counts)) <= 128  # every chunk's block-rows fit the 1024-row window
    nr = 8 * (counts[-1][0] + 2)
    r, c = cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32)
    v = np.random.default_rng(seed).uniform(0.1, 1.0, len(cells))
    A = bmsp.BmSpMatrix.from_coo(nr, NC, r, c, v)
    assert bmsp.spmv_launch_info(A)["kernel"] == "spmv_chunk_kernel"
    x = gen.spmv_x(NC, "cusp")
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
    y_ref = oracle.spmv_f32(oracle.bmsp_from_coo(oracle.Coo(nr, NC, r, c, v), 0, False), x)
    S = util.scipy_csr(nr, NC, r, c, np.asarray(v, np.float32).astype(np.float64))
    bound = 1e-5 * (abs(S) @ np.abs(x.astype(np.float64))) + 1e-30
    assert np.all(np.abs(ys[0] - y_ref) <= bound + 1e-5 * np.abs(y_ref)), np.max(np.abs(ys[0] - y_ref))


def seq(sizes, start=0, gap=1):
    """consecutive block-rows start, start + gap, ... with the given value counts"""
    return [(start + gap * i, k) for i, k in enumerate(sizes)]


# block-rows ending exactly on lane boundaries: 8, 16, 24 and 40 values, so every lane holds one block-row and runs cross lanes
LANE_ALIGNED = seq([8, 16, 24, 40] * 40)
# lanes with three and more block-rows: a lane of block-rows of 2 + 1 + 3 + 2 values, then a lane of 1 x 8, then block-rows that straddle
MANY_PER_LANE = seq([2, 1, 3, 2] + [1] * 8 + [5, 7, 4, 11, 3, 2] * 3 + [30] * 3)
# a block-row from lane 0 to lane 63: block-row 1 fills chunk 1 but its last 3 values, block-row 2 holds those 3 (chunk 0: block-row 0)
FULL_SPAN = [(0, V), (1, V - 3), (2, 3), (3, 700), (4, 61)]
# every lane its own block-row, 64 block-rows per chunk
LANE_EACH = seq([8] * (64 * 3 + 17))
# empty block-rows inside the window: every other block-row present
GAPS = seq([5, 9, 3, 17, 8, 1, 2, 26, 40] * 20, gap=2)


def extend(counts, reps):
    """the same pattern again `reps` times, behind the last block-row, so that the cases fall in every position of several chunks"""
    out, off = [], 0
    span = counts[-1][0] + 1
    for _ in range(reps):
        out += [(b + off, k) for b, k in counts]
        off += span
    return out


@pytest.mark.gpu
def test_lane_aligned_block_rows(oracle, bmsp, force_chunks):
    run(oracle, bmsp, LANE_ALIGNED, 31)


@pytest.mark.gpu
def test_many_block_rows_per_lane(oracle, bmsp, force_chunks):
    run(oracle, bmsp, extend(MANY_PER_LANE, 8), 32)


@pytest.mark.gpu
def test_block_row_across_all_lanes(oracle, bmsp, force_chunks):
    run(oracle, bmsp, FULL_SPAN, 33)


@pytest.mark.gpu
def test_every_lane_its_own_block_row(oracle, bmsp, force_chunks):
    run(oracle, bmsp, LANE_EACH, 34)


@pytest.mark.gpu
def test_empty_block_rows_in_window(oracle, bmsp, force_chunks):
    run(oracle, bmsp, GAPS, 35)


SHIFTS = [1, 3, 8, 13, 64, 509]


def mixed(shift):
    """every shape behind `shift` values in block-row 0: lane and chunk boundaries move through every segment case"""
    counts = [(0, shift)]
    for part in (LANE_ALIGNED[:24], MANY_PER_LANE, FULL_SPAN[1:], LANE_EACH[:70], GAPS[:40]):
        base = counts[-1][0] + 1 - part[0][0]
        counts += [(b + base, k) for b, k in part]
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
def test_shifted_mix(oracle, bmsp, force_chunks, shift):
    run(oracle, bmsp, mixed(shift), 40 + shift)


def test_layouts_hold_the_cases():
    ln = lanes(LANE_ALIGNED)
    assert all(np.unique(b).size == 1 for b in ln.values())
    assert sum(k for _, k in LANE_ALIGNED) % V != 0  # the partial last chunk
    assert max(np.unique(b).size for b in lanes(MANY_PER_LANE).values()) == 8
    ln = lanes(FULL_SPAN)
    assert all(ln[(1, l)][0] == 1 for l in range(64)) and ln[(1, 63)][-1] == 2
    ln = lanes(LANE_EACH)
    assert all(b[0] == b[-1] for b in ln.values()) and len({int(b[0]) for b in ln.values()}) == len(ln)
    assert GAPS[1][0] - GAPS[0][0] == 2
    for counts in (LANE_ALIGNED, extend(MANY_PER_LANE, 8), FULL_SPAN, LANE_EACH, GAPS) + tuple(mixed(s) for s in SHIFTS):
        assert max(windows(counts)) <= 128
