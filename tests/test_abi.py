"""CPU tests: the C-ABI library loads and exports every symbol include/bmsp.h declares; the host-only
entry points (MatrixMarket -> CSR) behave; errors are reported, never swallowed."""
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import REPO, MTX


def header_symbols():
    text = open(os.path.join(REPO, "include", "bmsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bmsp_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(bmsp):
    L = bmsp.lib()
    declared = header_symbols()
    assert len(declared) >= 30
    for s in declared:
        assert hasattr(L, s), "libbmsp.so does not export %s" % s
    assert sorted(bmsp.SYMBOLS) == declared
    assert b"gfx950" in L.bmsp_version()


def test_host_csr_reader_matches_cusp_semantics(bmsp, oracle):
    for rel in ("test/coordinate_pattern_symmetric.mtx", "test/coordinate_real_general.mtx", "laplacian/5pt_10x10.mtx",
                "random_10x10/000_nonzeros.mtx", "random_10x10/030_nonzeros.mtx"):
        path = os.path.join(MTX, rel)
        m = bmsp.CSRMatrix.from_mtx(path)
        nr, nc, ro, cols, vals = m.arrays()
        ref = oracle.csr_from_coo(oracle.mtx_read(path, strict=True))
        assert (nr, nc) == (ref.num_rows, ref.num_cols)
        np.testing.assert_array_equal(ro, ref.row_offsets)
        np.testing.assert_array_equal(cols, ref.cols)
        np.testing.assert_array_equal(vals, ref.vals)
    # suffix handling of the drop-in CLI: "name" and "name.mtx" both resolve (SPMV.cu:257,270)
    m = bmsp.CSRMatrix.from_mtx(os.path.join(MTX, "real", "A_matrix"))
    assert m.arrays()[0] == 24


def test_errors_are_reported(bmsp):
    with pytest.raises(bmsp.BmspError) as e:
        bmsp.CSRMatrix.from_mtx("/nonexistent/file")
    assert e.value.status == -2 and "cannot open" in str(e.value)
    bad = os.path.join(REPO, "tests", "golden", "ragusa16_known.json")
    with pytest.raises(bmsp.BmspError):
        bmsp.CSRMatrix.from_mtx(bad)
    with pytest.raises(bmsp.BmspError):
        bmsp.CSRMatrix.from_arrays(2, 2, [0, 1, 2], [0, 5], [1.0, 1.0])  # column out of range


def test_host_bit_helpers_against_bruteforce(tmp_path):
    exe = str(tmp_path / "bits")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-include", "cmath", os.path.join(REPO, "tests", "host_bits_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout


def test_host_mac_choice_table(tmp_path):
    """the block-MAC rule (csrc/mac_choice.h, no HIP) on both sides of every boundary, from facts built by hand"""
    exe = str(tmp_path / "mac_choice")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(REPO, "tests", "host_mac_choice_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout


def test_host_solve_schedule(tmp_path):
    """the iteration cap and the batches between two read-backs of a solve (csrc/solve_schedule.h, no HIP): the ramp, a fixed check, the
    cut at the cap, NO_CHECK's single batch"""
    exe = str(tmp_path / "solve_schedule")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(REPO, "tests", "host_solve_schedule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout


def test_host_handle_lifetimes(tmp_path):
    """what a handle caches (csrc/matrix.h, no HIP linked) against a counting pool: the two resets of bmsp_matrix_invalidate, re-assigned
    owners, delete with either ownership, buffers moved out; and the program filled as many owners as the struct declares"""
    from test_structure_invalidate import scan_handle
    exe = str(tmp_path / "handle")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(REPO, "tests", "host_handle_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout
    owning = scan_handle()[0]
    allocations = sum({"spmv_op_views": 2, "spsv_plans": 4, "shard_view": 0}.get(f, 1) for f in owning)
    assert out.stdout.split() == ["OK", "owners=%d" % allocations], (out.stdout, sorted(owning))


def _build_cpp_api_check(out_path):
    lib_dir = os.path.join(REPO, "bmsparse-spgemm-spmv_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "cpp_api_check.cpp"),
                           "-o", out_path, "-L" + lib_dir, "-lbmsp", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_headers_compile_and_link(tmp_path):
    """include/bmSpMatrix.h + include/CSRMatrix.h: every template the reference's mains and checks use instantiates and links
    against libbmsp.so with a plain host compiler (no HIP headers on the include path)."""
    _build_cpp_api_check(str(tmp_path / "cpp_api_check"))


def test_generators_are_deterministic():
    from pybmsp import gen
    n, _, r, c, v = gen.rmat(10, 4, seed=1)
    n2, _, r2, c2, v2 = gen.rmat(10, 4, seed=1)
    assert n == 1024 and r.size == c.size == v.size
    np.testing.assert_array_equal(r, r2); np.testing.assert_array_equal(c, c2); np.testing.assert_array_equal(v, v2)
    assert np.all(np.diff(r.astype(np.int64) * n + c) > 0)          # sorted, duplicates merged
    assert set(zip(range(n), range(n))) <= set(zip(r.tolist(), c.tolist()))  # identity present
    n, _, r, c, v = gen.banded(100, 3)
    assert r.size == 100 * 7 - 2 * (1 + 2 + 3) and np.all(np.abs(r - c) <= 3) and np.all(np.abs(v) <= 1)
    # splitmix64 known answer (seed 0 first output of the reference implementation)
    assert int(gen.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


def _write_mtx(path, n, nnz, seed, banner="%%MatrixMarket matrix coordinate real general"):
    rng = np.random.default_rng(seed)
    r = rng.integers(1, n + 1, nnz)
    c = rng.integers(1, n + 1, nnz)
    # number shapes seen in SuiteSparse files: short decimals, 16-17 significant digits, exponents, integers, negatives
    v = rng.standard_normal(nnz) * 10.0 ** rng.integers(-30, 30, nnz)
    fmt = rng.integers(0, 5, nnz)
    with open(path, "w") as f:
        f.write(banner + "\n% comment\n%\n")
        f.write("%d %d %d\n" % (n, n, nnz))
        txt = []
        for i in range(nnz):
            s = ["%.3f" % (v[i] % 1000), "%.17g" % v[i], "%.15e" % v[i], "%d" % int(v[i] % 1000), "%r" % float(v[i])][fmt[i]]
            txt.append("%d %d %s\n" % (r[i], c[i], s) if i % 7 else "  %d\t%d   %s \n" % (r[i], c[i], s))
        f.write("".join(txt))
    return r, c


def test_parallel_parser_matches_python_float(bmsp, tmp_path, monkeypatch):
    """the multi-threaded MatrixMarket reader (exact fast path + strtod fallback) against Python's float() on every token,
    single-threaded and 7-threaded, via the host-only CSR entry point."""
    path = str(tmp_path / "rand.mtx")
    n, nnz = 5000, 200000
    _write_mtx(path, n, nnz, 11)
    toks = [l.split() for l in open(path).read().splitlines()[4:]]
    rows = np.array([int(t[0]) - 1 for t in toks]); cols = np.array([int(t[1]) - 1 for t in toks])
    vals = np.array([float(t[2]) for t in toks])
    order = np.lexsort((cols, rows))  # stable (row, col) sort like the CUSP reader
    with np.errstate(over="ignore"):
        ref_vals = vals[order].astype(np.float32)
    results = []
    for threads in ("1", "7"):
        monkeypatch.setenv("BMSP_PARSE_THREADS", threads)
        nr, nc, ro, ci, v = bmsp.CSRMatrix.from_mtx(path).arrays()
        assert (nr, nc, ci.size) == (n, n, nnz)
        np.testing.assert_array_equal(ci, cols[order])
        np.testing.assert_array_equal(v.view(np.uint32), ref_vals.view(np.uint32))
        results.append((ro, ci, v))
    np.testing.assert_array_equal(results[0][0], results[1][0])
    # truncated and over-long bodies are errors, not silent garbage
    lines = open(path).read().splitlines(True)
    open(path, "w").write("".join(lines[:-5]))
    with pytest.raises(bmsp.BmspError):
        bmsp.CSRMatrix.from_mtx(path)
    open(path, "w").write("".join(lines + ["1 1 1.0\n"]))
    with pytest.raises(bmsp.BmspError):
        bmsp.CSRMatrix.from_mtx(path)


def test_csr_host_path_matches_cusp_semantics(bmsp, oracle):
    """configs[0]: CSRMatrix's host path (bmsp_csr_spmv_host / bmsp_csr_multiply_host, no GPU call) on the reference-held fixtures
    and the cusp multiply.cu known answers: SpMV bit-identical with the oracle's restatement of csr_spmv.h:56-73 (same summation
    order), products equal the dense product and drop numeric zeros like csr_spgemm.h:135; 1 thread and several."""
    import json
    from conftest import GOLDEN
    for rel in ("laplacian/5pt_10x10.mtx", "laplacian/7pt_10x10x10.mtx", "random_10x10/030_nonzeros.mtx", "random_10x10/000_nonzeros.mtx", "real/A_matrix.mtx"):
        path = os.path.join(MTX, rel)
        m = bmsp.CSRMatrix.from_mtx(path)
        nr, nc, ro, cols, vals = m.arrays()
        ref = oracle.csr_from_coo(oracle.mtx_read(path, strict=True))
        x = (np.arange(nc) % 10).astype(np.float32)
        want = oracle.csr_spmv(ref, x, 1)
        for th in (1, 3):
            np.testing.assert_array_equal(m.spmv_host(x, th).view(np.uint32), want.view(np.uint32))
        if nr == nc:
            dense = np.zeros((nr, nc))
            for i in range(nr):
                dense[i, cols[ro[i]:ro[i + 1]]] = vals[ro[i]:ro[i + 1]]
            for th in (1, 4):
                c = m.multiply_host(m, th)
                cr, cc, cro, ccols, cvals = c.arrays()
                got = np.zeros((cr, cc))
                for i in range(cr):
                    assert len(set(ccols[cro[i]:cro[i + 1]].tolist())) == cro[i + 1] - cro[i]
                    got[i, ccols[cro[i]:cro[i + 1]]] = cvals[cro[i]:cro[i + 1]]
                np.testing.assert_array_equal(got, dense @ dense)
                assert not np.any(cvals == 0.0)
    g = json.load(open(os.path.join(GOLDEN, "cusp_multiply.json")))
    import scipy.sparse as sp
    for pr in g["products"]:
        L = np.asarray(g["matrices"][pr["left"]]["dense"], dtype=np.float32)
        R = np.asarray(g["matrices"][pr["right"]]["dense"], dtype=np.float32)
        la, ra = sp.csr_matrix(L), sp.csr_matrix(R)
        la.sort_indices(); ra.sort_indices()
        a = bmsp.CSRMatrix.from_arrays(L.shape[0], L.shape[1], la.indptr, la.indices, la.data)
        b = bmsp.CSRMatrix.from_arrays(R.shape[0], R.shape[1], ra.indptr, ra.indices, ra.data)
        cr, cc, cro, ccols, cvals = a.multiply_host(b, 2).arrays()
        got = sp.csr_matrix((cvals, ccols, cro), shape=(cr, cc)).toarray().astype(np.float64)
        np.testing.assert_array_equal(got, np.asarray(pr["dense"], dtype=np.float64))


def test_comm_rendezvous_argument_errors(bmsp, monkeypatch):
    """bmsp_comm_init_from_env / bmsp_comm_init reject bad rendezvous settings before RCCL is touched (runs without a GPU)."""
    import ctypes
    h = ctypes.c_void_p()
    monkeypatch.delenv("BMSP_WORLD", raising=False)
    monkeypatch.delenv("BMSP_RANK", raising=False)
    assert bmsp.lib().bmsp_comm_init_from_env(ctypes.byref(h)) == -1 and b"BMSP_WORLD" in bmsp.lib().bmsp_last_error()
    monkeypatch.setenv("BMSP_WORLD", "4"); monkeypatch.setenv("BMSP_RANK", "7")
    assert bmsp.lib().bmsp_comm_init_from_env(ctypes.byref(h)) == -1 and b"outside" in bmsp.lib().bmsp_last_error()
    monkeypatch.setenv("BMSP_RANK", "1"); monkeypatch.delenv("BMSP_COMM_FILE", raising=False)
    assert bmsp.lib().bmsp_comm_init_from_env(ctypes.byref(h)) == -1 and b"BMSP_COMM_FILE" in bmsp.lib().bmsp_last_error()
    with pytest.raises(bmsp.BmspError):
        bmsp.Comm(b"\0" * 128, 2, 5)
    assert bmsp.lib().bmsp_comm_free(None) == 0
