"""The carry hand-off of the chunked SpMV sweep (spmv_chunk_kernel) at the fold widths and slot patterns its code paths split on: one
ticket instruction for a chunk's head and tail slots, and a fold that loads up to 8 / 16 / 32 chunks' slots per batch before it waits
(longer spans take several batches); hub chunks (one block-row) and window chunks both park slots.  Every case forces the chunked
sweep, poisons y with NaN, requires repeated sweeps to be bitwise equal and checks against the oracle (test_spmv_chunk_folds.run); the
last case repeats the long-fold layout in queued launches with changing x (test_fold_history)."""
import numpy as np
import pytest
from test_fold_history import Case, run_history
from test_spmv_chunk_folds import V, chunks_of, run

pytestmark = pytest.mark.gpu

NBC = 8192  # block columns of the test matrices (65536 columns): a block-row holds up to 65536 values


@pytest.fixture
def force_chunks(monkeypatch):
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")


def cells_of(counts, seed):
    """counts: {block-row: stored values}; distinct columns (several values per tile where a block-row is long), rows spread over the
    block-row's 8 rows"""
    g = np.random.default_rng(seed)
    cells = []
    for br, k in counts.items():
        cols = np.sort(g.choice(8 * NBC, k, replace=False))
        cells.append(np.stack([8 * br + g.integers(0, 8, k), cols], axis=1))
    return np.concatenate(cells).astype(np.int64)


def spans(counts):
    """{block-row: number of 512-value chunks its values lie in}"""
    out, o = {}, 0
    for br, k in counts.items():
        out[br] = (o + k - 1) // V - o // V + 1
        o += k
    return out


def chain(widths, gap=37, first=100):
    """block-rows spanning widths[i] chunks each, one after the other, separated by a block-row of `gap` values (so the chunk that ends
    one fold also starts the next: a head and a tail slot); block-row 0 holds `first` values"""
    counts, o, br = {0: first}, first, 1
    for n in widths:
        k = (V - o % V) + V * (n - 2) + 100  # to the end of its first chunk, n - 2 whole chunks, 100 values into the last
        counts[br] = k
        o += k
        counts[br + 1] = gap
        o += gap
        br += 2
    return counts


def rows_of(counts):
    return 8 * (max(counts) + 1)


def test_long_fold_past_batches(oracle, bmsp, force_chunks):
    # one block-row over 46 chunks (two batches of loads, the second partial) and one over 41, between short block-rows
    counts = {0: 100, 1: 45 * V - 63, 2: 300, 3: 50, 4: 40 * V + 5, 5: 20}
    sp = spans(counts)
    assert sp[1] == 46 and sp[4] == 41
    run(oracle, bmsp, rows_of(counts), 8 * NBC, cells_of(counts, 31), 31)


@pytest.mark.parametrize("widths", [(2, 3, 8, 9, 16, 17), (32, 33, 2, 65)], ids=["2-17", "32-65"])
def test_fold_widths(oracle, bmsp, force_chunks, widths):
    # every width at a batch edge of the fold: 8 (one load per lane), 16 (two), 32 (a batch of four), 33 and 65 (one slot past a batch)
    counts = chain(widths)
    sp = spans(counts)
    assert [sp[2 * i + 1] for i in range(len(widths))] == list(widths)
    ch = chunks_of(counts)
    assert sum(h and t for h, t, _ in ch) == len(widths) - 1  # each gap chunk ends one fold and starts the next
    run(oracle, bmsp, rows_of(counts), 8 * NBC, cells_of(counts, 32 + len(widths)), 32 + len(widths))


def test_runs_of_both_slots(oracle, bmsp, force_chunks):
    # block-rows of 300 .. 700 values back to back: runs of chunks with a head and a tail slot, two- and three-way folds
    g = np.random.default_rng(41)
    counts = {br: int(g.integers(300, 700)) for br in range(200)}
    ch = chunks_of(counts)
    both = [h and t for h, t, _ in ch]
    run_len = max(len(s) for s in "".join("b" if b else "." for b in both).split("."))
    assert run_len >= 20, run_len
    run(oracle, bmsp, rows_of(counts), 8 * NBC, cells_of(counts, 41), 41)


def test_hub_then_sparse_rows(oracle, bmsp, force_chunks):
    # a hub block-row of 12 chunks (hub chunks park one slot each: the first a tail, the rest heads) followed by 400 block-rows of a
    # few values: the window chunk behind the hub holds its head block-row
    g = np.random.default_rng(42)
    counts = {0: 12 * V - 200}
    counts.update({br: int(g.integers(1, 30)) for br in range(1, 400)})
    ch = chunks_of(counts)
    assert ch[0] == (False, True, True) and all(c == (True, False, True) for c in ch[1:11]) and ch[11][0] and not ch[11][2]
    run(oracle, bmsp, rows_of(counts), 8 * NBC, cells_of(counts, 42), 42)


@pytest.mark.parametrize("last", [3 * V + 77, 2 * V + 400, 40])
def test_partial_last_chunk_in_fold(oracle, bmsp, force_chunks, last):
    # the last block-row is folded and ends inside the partial last chunk: that chunk is a hub chunk holding only its end (first two
    # cases) or, with a 40-value last block-row, a window chunk whose fold ends on the block-row before
    counts = {br: 300 for br in range(8)}
    counts[8] = 5 * V + 11
    counts[9] = last
    ch = chunks_of(counts)
    total = sum(counts.values())
    assert total % V != 0 and ch[-1][0] and not ch[-1][1]
    run(oracle, bmsp, rows_of(counts) + 5, 8 * NBC, cells_of(counts, 43), 43)


def test_long_fold_history(oracle, bmsp, monkeypatch):
    # the long-fold layout in queued launches with changing x (every input after every other), then new values
    monkeypatch.setenv("BMSP_SPMV_CHUNK", "1")
    counts = {0: 100, 1: 45 * V - 63, 2: 300, 3: 50, 4: 17 * V, 5: 20}
    cells = np.unique(cells_of(counts, 44), axis=0)
    r, c = cells[:, 0].astype(np.int32), cells[:, 1].astype(np.int32)
    v = np.random.default_rng(44).uniform(0.1, 1.0, len(cells))
    case = Case(bmsp, oracle, rows_of(counts), 8 * NBC, r, c, v, seed=4)
    assert bmsp.spmv_launch_info(case.A)["kernel"] == "spmv_chunk_kernel"
    run_history(case, 4, bitwise=True, values=True, kernel="spmv_chunk_kernel")
