"""pybmsp -- thin ctypes binding of libbmsp.so (include/bmsp.h), used by tests/ and bench.py.

Plumbing only: every operation is a call through the C ABI into the HIP kernels.  There is no CPU fallback;
if the shared library is missing or a call fails, an exception is raised.

If PyTorch is used in the same process, import torch BEFORE this module so that both share one HIP runtime
(torch/lib/libamdhip64.so and /opt/rocm/lib/libamdhip64.so carry the same SONAME).
"""
import ctypes as C
import os
import subprocess
import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BMSP_LIB_PATH") or os.path.join(_PKG, "lib", "libbmsp.so")  # (the override: A/B runs of two builds in one GPU session)

F32, F16, F64 = 0, 1, 2
NP_DTYPE = {F32: np.float32, F16: np.float16, F64: np.float64}
OUT_DTYPE = {F32: np.float32, F16: np.float32, F64: np.float64}
SORT_AUTO, SORT_SEGMENTED, SORT_GLOBAL = 0, 1, 2
SPMV_DEFAULT, SPMV_BATCHED = 0, 1
PRUNE_ABS, PRUNE_ROW_REL = 0, 1
PRUNE_KEEP_DIAGONAL = 1
SELECT_COMPLEMENT = 1
BAND_MIN, BAND_MAX = -(1 << 63), (1 << 63) - 1
SCALE_DIV_LEFT, SCALE_DIV_RIGHT = 1, 2
OP_N, OP_T = 0, 1
SDDMM_MUL_S = 1
MASKED_MUL_M = 1
FILL_LOWER, FILL_UPPER = 0, 1
DIAG_NON_UNIT, DIAG_UNIT = 0, 1
ITSV_X0_GIVEN = 1
ITSV_NO_CHECK = -1.0
ILU_F0_GIVEN = 1
ILU_NO_CHECK = -1.0
KRYLOV_CG, KRYLOV_BICGSTAB = 0, 1
PC_NONE, PC_JACOBI, PC_ILU_EXACT, PC_ILU_SWEEPS = 0, 1, 2, 3
KRYLOV_X0_GIVEN = 1
KRYLOV_NO_CHECK = -1.0
KRYLOV_MAXITER, KRYLOV_CONVERGED, KRYLOV_BREAKDOWN = 0, 1, 2
MG_MAX_LEVELS = 16
MG_RESTRICT_ROW, MG_RESTRICT_SPMV, MG_RESTRICT_PT = 0, 1, 2
FSAI_SCALE_NONE, FSAI_SCALE_SQRT, FSAI_SCALE_UNIT = 0, 1, 2
FSAI_SPD, FSAI_GENERAL = 0, 1
FSAI_NO_MATERIALISE, FSAI_COLMAJOR = 1, 2
_METHODS = {"cg": KRYLOV_CG, "bicgstab": KRYLOV_BICGSTAB, KRYLOV_CG: KRYLOV_CG, KRYLOV_BICGSTAB: KRYLOV_BICGSTAB}
_FSAI_SCALES = {"none": FSAI_SCALE_NONE, "sqrt": FSAI_SCALE_SQRT, "unit": FSAI_SCALE_UNIT, 0: 0, 1: 1, 2: 2}
_FSAI_KINDS = {"spd": FSAI_SPD, "general": FSAI_GENERAL, 0: 0, 1: 1}
_OPS = {"N": OP_N, "T": OP_T, "n": OP_N, "t": OP_T, OP_N: OP_N, OP_T: OP_T}
_FILLS = {"lower": FILL_LOWER, "upper": FILL_UPPER, "L": FILL_LOWER, "U": FILL_UPPER, FILL_LOWER: FILL_LOWER, FILL_UPPER: FILL_UPPER}
_PRUNE_RULES = {"abs": PRUNE_ABS, "row_rel": PRUNE_ROW_REL, PRUNE_ABS: PRUNE_ABS, PRUNE_ROW_REL: PRUNE_ROW_REL}

# every symbol include/bmsp.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "bmsp_last_error", "bmsp_version", "bmsp_device_count", "bmsp_set_device", "bmsp_malloc", "bmsp_free",
    "bmsp_memcpy_h2d", "bmsp_memcpy_d2h", "bmsp_memcpy_d2d", "bmsp_memset", "bmsp_synchronize", "bmsp_trim_pool",
    "bmsp_event_create", "bmsp_event_record", "bmsp_event_elapsed_ms", "bmsp_event_destroy",
    "bmsp_matrix_from_mtx", "bmsp_matrix_from_coo", "bmsp_matrix_from_coo_device", "bmsp_matrix_from_arrays",
    "bmsp_matrix_save", "bmsp_matrix_load", "bmsp_matrix_free", "bmsp_matrix_prepare", "bmsp_matrix_invalidate", "bmsp_matrix_info", "bmsp_matrix_arrays", "bmsp_matrix_block_row_ptr",
    "bmsp_matrix_transpose", "bmsp_matrix_convert_layout", "bmsp_matrix_copy_values", "bmsp_matrix_add", "bmsp_matrix_add_values",
    "bmsp_matrix_prune", "bmsp_matrix_row_absmax", "bmsp_matrix_select_band", "bmsp_matrix_select_mask",
    "bmsp_matrix_diagonal", "bmsp_matrix_from_diagonal", "bmsp_matrix_scale", "bmsp_matrix_scale_values",
    "bmsp_matrix_to_coo_host", "bmsp_matrix_to_coo_device", "bmsp_matrix_to_csr_device", "bmsp_matrix_from_csr_device", "bmsp_matrix_compare", "bmsp_matrix_compare_device", "bmsp_spmv", "bmsp_spmv_launch_info", "bmsp_spmv_chunk_layout", "bmsp_spmv_op", "bmsp_spmv_op_launch_info", "bmsp_spmv_op_plan_items", "bmsp_spsv_analyse", "bmsp_spsv", "bmsp_spsv_plan", "bmsp_spsm", "bmsp_spsm_launch_info", "bmsp_spitsv", "bmsp_matrix_ilu0", "bmsp_matrix_ilu0_values", "bmsp_vec_dot", "bmsp_vec_axpby", "bmsp_matrix_color_blocks", "bmsp_matrix_permute_blocks", "bmsp_vec_permute_blocks", "bmsp_matrix_aggregate", "bmsp_matrix_from_aggregates", "bmsp_krylov_solve", "bmsp_gmres_solve", "bmsp_mg_create", "bmsp_mg_free", "bmsp_mg_info", "bmsp_mg_vcycle", "bmsp_mg_solve", "bmsp_mg_solve_gmres", "bmsp_matrix_fsai", "bmsp_matrix_fsai_values", "bmsp_fsai_create", "bmsp_fsai_update", "bmsp_fsai_free", "bmsp_fsai_get_info", "bmsp_fsai_factors", "bmsp_fsai_apply", "bmsp_fsai_solve", "bmsp_fsai_solve_gmres", "bmsp_sddmm", "bmsp_sddmm_values", "bmsp_sddmm_launch_info", "bmsp_spgemm_masked", "bmsp_spgemm_masked_values", "bmsp_spgemm_masked_launch_info", "bmsp_spmm", "bmsp_spmm_launch_info", "bmsp_spmm_op", "bmsp_spmm_op_launch_info", "bmsp_spgemm", "bmsp_spgemm_symbolic", "bmsp_spgemm_numeric", "bmsp_selftest_mfma_layout", "bmsp_selftest_mfma_f32_chain", "bmsp_selftest_tile_product", "bmsp_selftest_mfma_f32_cancel", "bmsp_segsort_u64",
    "bmsp_partition_rows", "bmsp_matrix_row_panel", "bmsp_matrix_concat_panels",
    "bmsp_comm_unique_id", "bmsp_comm_init", "bmsp_comm_init_from_env", "bmsp_comm_init_loopback", "bmsp_shard_layout", "bmsp_shard_row_slices", "bmsp_comm_info", "bmsp_comm_free", "bmsp_spgemm_sharded", "bmsp_spgemm_sharded_ex", "bmsp_spmv_sharded",
    "bmsp_csr_from_mtx", "bmsp_csr_from_arrays", "bmsp_csr_info", "bmsp_csr_arrays", "bmsp_csr_multiply",
    "bmsp_csr_spmv", "bmsp_csr_multiply_host", "bmsp_csr_spmv_host", "bmsp_csr_free",
]


class BmspError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("bmsp status %d: %s" % (status, msg))
        self.status = status


class SpgemmStats(C.Structure):
    _fields_ = [("task_list_size", C.c_int64), ("bmp_reduction", C.c_int64), ("surviving_tasks", C.c_int64),
                ("c_blocks", C.c_int64), ("c_nnz", C.c_int64), ("t_us", C.c_double * 10),
                ("sort_path", C.c_int), ("mac_kernel", C.c_int), ("mac_variant", C.c_int), ("sort_long", C.c_int)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("task_list_size", "bmp_reduction", "surviving_tasks", "c_blocks", "c_nnz",
                                           "sort_path", "mac_kernel", "mac_variant", "sort_long")}
        d["t_us"] = list(self.t_us)
        return d


class PruneStats(C.Structure):
    _fields_ = [("nnz_in", C.c_int64), ("nnz_out", C.c_int64), ("blocks_in", C.c_int64), ("blocks_out", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SelectStats = PruneStats  # bmsp_select_stats is bmsp_prune_stats


class SpmvOpInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("slots", C.c_int), ("items", C.c_int64), ("split_blocks", C.c_int64), ("view_bytes", C.c_int64),
                ("compulsory_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class SpmmOpInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("col_chunks", C.c_int), ("items", C.c_int64), ("split_blocks", C.c_int64),
                ("view_bytes", C.c_int64), ("scratch_bytes", C.c_int64), ("compulsory_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class SddmmInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("compulsory_bytes", C.c_int64)]

    def as_dict(self):
        return {"kernel": self.kernel.decode(), "lanes": self.lanes, "compulsory_bytes": self.compulsory_bytes}


class SpgemmMaskedInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("pairs", C.c_int64), ("view_bytes", C.c_int64)]

    def as_dict(self):
        return {"kernel": self.kernel.decode(), "lanes": self.lanes, "pairs": self.pairs, "view_bytes": self.view_bytes}


class SpsvInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("levels", C.c_int64), ("max_level_width", C.c_int64), ("launches", C.c_int64),
                ("chain_launches", C.c_int64), ("chained_levels", C.c_int64), ("plan_bytes", C.c_int64)]

    def as_dict(self):
        return {"kernel": self.kernel.decode(), "levels": self.levels, "max_level_width": self.max_level_width, "launches": self.launches,
                "chain_launches": self.chain_launches, "chained_levels": self.chained_levels, "plan_bytes": self.plan_bytes}


class SpsmInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("col_chunks", C.c_int), ("levels", C.c_int64), ("launches", C.c_int64),
                ("chain_launches", C.c_int64), ("chained_levels", C.c_int64), ("plan_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class SpitsvInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("sweeps", C.c_int64), ("levels", C.c_int64), ("converged", C.c_int), ("delta", C.c_double),
                ("xmax", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class Ilu0Info(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("sweeps", C.c_int64), ("max_sweeps", C.c_int64), ("converged", C.c_int),
                ("delta", C.c_double), ("fmax", C.c_double), ("view_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class ColorInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("blocks", C.c_int64), ("colors", C.c_int64), ("rounds", C.c_int64), ("view_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class AggregateInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("nodes", C.c_int64), ("aggregates", C.c_int64), ("rounds", C.c_int64), ("launches", C.c_int64),
                ("view_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class Precond(C.Structure):
    _fields_ = [("kind", C.c_int), ("F", C.c_void_p), ("sweeps", C.c_int64)]


class KrylovInfo(C.Structure):
    _fields_ = [("method", C.c_char * 32), ("iterations", C.c_int64), ("max_iterations", C.c_int64), ("status", C.c_int),
                ("relres", C.c_double), ("bnorm", C.c_double), ("products", C.c_int64), ("precond_applies", C.c_int64),
                ("workspace_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["method"] = self.method.decode()
        return d


class MgInfo(C.Structure):
    _fields_ = [("levels", C.c_int), ("pre", C.c_int), ("post", C.c_int), ("coarse_exact", C.c_int), ("n", C.c_int64 * MG_MAX_LEVELS),
                ("restrict_mode", C.c_int * MG_MAX_LEVELS), ("kernel", C.c_char * 64), ("coarse_kernel", C.c_char * 64),
                ("workspace_bytes", C.c_int64), ("launches_per_cycle", C.c_int64)]

    def as_dict(self):
        return {"levels": self.levels, "pre": self.pre, "post": self.post, "coarse_exact": self.coarse_exact,
                "n": list(self.n)[:self.levels], "restrict_mode": list(self.restrict_mode)[:max(self.levels - 1, 0)],
                "kernel": self.kernel.decode(), "coarse_kernel": self.coarse_kernel.decode(), "workspace_bytes": self.workspace_bytes,
                "launches_per_cycle": self.launches_per_cycle}


class FsaiInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lanes", C.c_int), ("rows", C.c_int64), ("max_row", C.c_int64), ("pairs", C.c_int64),
                ("bad_rows", C.c_int64), ("lds_bytes", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel"] = self.kernel.decode()
        return d


class FsaiHandleInfo(C.Structure):
    _fields_ = [("kind", C.c_int), ("flags", C.c_int), ("materialised", C.c_int), ("n", C.c_int64), ("owned_bytes", C.c_int64),
                ("factor", FsaiInfo * 2)]

    def as_dict(self):
        return {"kind": self.kind, "flags": self.flags, "materialised": self.materialised, "n": self.n, "owned_bytes": self.owned_bytes,
                "factor": [self.factor[0].as_dict(), self.factor[1].as_dict()]}


class ShardStats(C.Structure):
    _fields_ = [("world", C.c_int), ("rank", C.c_int), ("panel_block_row_begin", C.c_int64), ("panel_block_row_end", C.c_int64),
                ("panel_tasks", C.c_int64), ("exchange_bytes", C.c_int64), ("exchange_us", C.c_double), ("exchange_exposed_us", C.c_double),
                ("exchange_hidden_frac", C.c_double), ("rounds", C.c_int), ("gathered", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def build_library():
    subprocess.check_call(["make", "-s", "-C", _PKG, "lib"])
    return LIB_PATH


def lib():
    """loads libbmsp.so; fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libbmsp.so not built: run `make -C %s lib` (or __graft_entry__.build())" % _PKG)
        L = C.CDLL(LIB_PATH)
        L.bmsp_last_error.restype = C.c_char_p
        L.bmsp_version.restype = C.c_char_p
        p, i, i64, vp = C.POINTER, C.c_int, C.c_int64, C.c_void_p
        L.bmsp_malloc.argtypes = [p(vp), C.c_size_t]
        L.bmsp_free.argtypes = [vp]
        L.bmsp_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
        L.bmsp_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
        L.bmsp_memcpy_d2d.argtypes = [vp, vp, C.c_size_t]
        L.bmsp_memset.argtypes = [vp, i, C.c_size_t]
        L.bmsp_event_create.argtypes = [p(vp)]
        L.bmsp_event_record.argtypes = [vp, vp]
        L.bmsp_event_elapsed_ms.argtypes = [vp, vp, p(C.c_float)]
        L.bmsp_event_destroy.argtypes = [vp]
        L.bmsp_matrix_from_mtx.argtypes = [C.c_char_p, i, i, p(vp)]
        L.bmsp_matrix_from_coo.argtypes = [i, i, i64, vp, vp, vp, i, i, p(vp)]
        L.bmsp_matrix_from_coo_device.argtypes = [i, i, i64, vp, vp, vp, i, i, vp, p(vp)]
        L.bmsp_matrix_from_arrays.argtypes = [i, i, i64, i64, vp, vp, vp, vp, i, i, i, p(vp)]
        L.bmsp_matrix_save.argtypes = [vp, C.c_char_p]
        L.bmsp_matrix_load.argtypes = [C.c_char_p, p(vp)]
        L.bmsp_matrix_free.argtypes = [vp]
        L.bmsp_matrix_prepare.argtypes = [vp, i, vp]
        L.bmsp_matrix_info.argtypes = [vp, p(i), p(i), p(i64), p(i64), p(i), p(i)]
        L.bmsp_matrix_arrays.argtypes = [vp, p(vp), p(vp), p(vp), p(vp)]
        L.bmsp_matrix_block_row_ptr.argtypes = [vp, p(vp), p(i64)]
        L.bmsp_matrix_transpose.argtypes = [vp, i, vp, p(vp)]
        L.bmsp_matrix_convert_layout.argtypes = [vp, i, vp, p(vp)]
        L.bmsp_matrix_copy_values.argtypes = [vp, vp, vp]
        L.bmsp_matrix_add.argtypes = [C.c_double, vp, C.c_double, vp, i, vp, p(vp)]
        L.bmsp_matrix_add_values.argtypes = [C.c_double, vp, C.c_double, vp, vp, vp]
        L.bmsp_matrix_prune.argtypes = [vp, i, C.c_double, i, i, vp, p(vp), p(PruneStats)]
        L.bmsp_matrix_row_absmax.argtypes = [vp, vp, vp]
        L.bmsp_matrix_select_band.argtypes = [vp, C.c_int64, C.c_int64, i, i, vp, p(vp), p(SelectStats)]
        L.bmsp_matrix_select_mask.argtypes = [vp, vp, i, i, vp, p(vp), p(SelectStats)]
        L.bmsp_matrix_diagonal.argtypes = [vp, vp, vp]
        L.bmsp_matrix_from_diagonal.argtypes = [i, i, vp, i, i, vp, p(vp)]
        L.bmsp_matrix_scale.argtypes = [vp, vp, vp, i, i, vp, p(vp)]
        L.bmsp_matrix_scale_values.argtypes = [vp, vp, vp, i, vp, vp]
        L.bmsp_matrix_to_coo_host.argtypes = [vp, vp, vp, vp]
        L.bmsp_matrix_to_coo_device.argtypes = [vp, vp, vp, vp, vp]
        L.bmsp_matrix_to_csr_device.argtypes = [vp, vp, vp, vp, vp]
        L.bmsp_matrix_from_csr_device.argtypes = [i, i, i64, vp, vp, vp, i, i, vp, p(vp)]
        L.bmsp_matrix_compare_device.argtypes = [vp, i64, vp, vp, vp, p(C.c_double), p(i64), vp]
        L.bmsp_matrix_compare.argtypes = [vp, i64, vp, vp, vp, p(C.c_double), p(i64)]
        L.bmsp_spmv.argtypes = [vp, vp, vp, i, vp]
        L.bmsp_spmm.argtypes = [vp, vp, i64, vp, i64, i, vp]
        L.bmsp_spmv_launch_info.argtypes = [vp, i, C.c_char_p, C.c_size_t, p(i64), p(i64)]
        L.bmsp_spmv_chunk_layout.argtypes = [vp, p(i)]
        L.bmsp_spmv_op.argtypes = [vp, i, C.c_double, vp, C.c_double, vp, vp]
        L.bmsp_spmv_op_launch_info.argtypes = [vp, i, p(SpmvOpInfo)]
        L.bmsp_spmv_op_plan_items.argtypes = [vp, i64, i64, vp, vp, p(i64), p(i64), p(i64)]
        L.bmsp_spsv_analyse.argtypes = [vp, i, i, i, vp, p(SpsvInfo)]
        L.bmsp_spsv.argtypes = [vp, i, i, i, C.c_double, vp, vp, vp]
        L.bmsp_spsv_plan.argtypes = [vp, vp, i64, i, i64, vp, vp, vp, vp, p(i64), p(i64)]
        L.bmsp_spsm.argtypes = [vp, i, i, i, C.c_double, vp, i64, vp, i64, i, vp]
        L.bmsp_spsm_launch_info.argtypes = [vp, i, i, i, i, i64, i64, vp, p(SpsmInfo)]
        L.bmsp_spitsv.argtypes = [vp, i, i, i, C.c_double, vp, vp, i64, C.c_double, i, vp, p(SpitsvInfo), vp]
        L.bmsp_matrix_ilu0.argtypes = [vp, i64, C.c_double, i, vp, p(vp), vp, p(Ilu0Info)]
        L.bmsp_matrix_ilu0_values.argtypes = [vp, vp, i64, C.c_double, i, vp, vp, p(Ilu0Info)]
        L.bmsp_vec_dot.argtypes = [i64, i, vp, vp, vp, vp]
        L.bmsp_vec_axpby.argtypes = [i64, i, C.c_double, vp, C.c_double, vp, vp]
        L.bmsp_matrix_color_blocks.argtypes = [vp, C.c_uint64, vp, vp, vp, p(ColorInfo)]
        L.bmsp_matrix_permute_blocks.argtypes = [vp, vp, vp, i, vp, p(vp)]
        L.bmsp_vec_permute_blocks.argtypes = [i64, i, vp, i, vp, vp, vp]
        L.bmsp_matrix_aggregate.argtypes = [vp, C.c_uint64, vp, p(i64), vp, p(AggregateInfo)]
        L.bmsp_matrix_from_aggregates.argtypes = [i, i, vp, vp, i, i, vp, p(vp)]
        L.bmsp_krylov_solve.argtypes =[vp, i, i, p(Precond), vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_gmres_solve.argtypes = [vp, i, p(Precond), i, vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_mg_create.argtypes = [i, vp, vp, vp, vp, i64, C.c_double, i, i, vp, p(vp)]
        L.bmsp_mg_free.argtypes = [vp]
        L.bmsp_mg_info.argtypes = [vp, p(MgInfo)]
        L.bmsp_mg_vcycle.argtypes = [vp, vp, vp, vp]
        L.bmsp_mg_solve.argtypes = [vp, i, vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_mg_solve_gmres.argtypes = [vp, i, vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_matrix_fsai.argtypes = [vp, i, vp, i, i, vp, vp, p(vp), p(FsaiInfo)]
        L.bmsp_matrix_fsai_values.argtypes = [vp, i, vp, i, vp, vp, p(FsaiInfo)]
        L.bmsp_fsai_create.argtypes = [vp, vp, i, i, vp, p(vp)]
        L.bmsp_fsai_update.argtypes = [vp, vp]
        L.bmsp_fsai_free.argtypes = [vp]
        L.bmsp_fsai_get_info.argtypes = [vp, p(FsaiHandleInfo)]
        L.bmsp_fsai_factors.argtypes = [vp, p(vp), p(vp)]
        L.bmsp_fsai_apply.argtypes = [vp, vp, vp, vp]
        L.bmsp_fsai_solve.argtypes = [vp, i, vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_fsai_solve_gmres.argtypes = [vp, i, vp, vp, i64, C.c_double, i, vp, p(KrylovInfo), vp]
        L.bmsp_sddmm.argtypes = [vp, vp, i64, vp, i64, i, C.c_double, C.c_double, i, i, vp, p(vp)]
        L.bmsp_sddmm_values.argtypes = [vp, vp, i64, vp, i64, i, C.c_double, C.c_double, i, vp, vp]
        L.bmsp_sddmm_launch_info.argtypes = [vp, i, i64, i64, i, p(SddmmInfo)]
        L.bmsp_spgemm_masked.argtypes = [vp, vp, vp, C.c_double, C.c_double, i, i, vp, p(vp)]
        L.bmsp_spgemm_masked_values.argtypes = [vp, vp, vp, C.c_double, C.c_double, i, vp, vp]
        L.bmsp_spgemm_masked_launch_info.argtypes = [vp, vp, vp, i, p(SpgemmMaskedInfo)]
        L.bmsp_spmm_launch_info.argtypes = [vp, i, i64, i64, C.c_char_p, C.c_size_t]
        L.bmsp_spmm_op.argtypes = [vp, i, C.c_double, vp, i64, C.c_double, vp, i64, i, vp]
        L.bmsp_spmm_op_launch_info.argtypes = [vp, i, i, i64, i64, p(SpmmOpInfo)]
        L.bmsp_spgemm.argtypes = [vp, vp, p(vp), i, i, i, vp, p(SpgemmStats)]
        L.bmsp_spgemm_symbolic.argtypes = [vp, vp, p(vp), i, i, vp, p(SpgemmStats)]
        L.bmsp_spgemm_numeric.argtypes = [vp, vp, vp, i, vp, p(SpgemmStats)]
        L.bmsp_selftest_mfma_layout.argtypes = [p(i)]
        L.bmsp_selftest_mfma_f32_chain.argtypes = [p(i)]
        L.bmsp_selftest_tile_product.argtypes = [p(i)]
        L.bmsp_selftest_mfma_f32_cancel.argtypes = [p(i), p(i)]
        L.bmsp_segsort_u64.argtypes = [vp, vp, i, i64, vp, i64, vp]
        L.bmsp_partition_rows.argtypes = [vp, vp, i, vp]
        L.bmsp_matrix_row_panel.argtypes = [vp, i64, i64, p(vp)]
        L.bmsp_matrix_concat_panels.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, i, p(vp)]
        L.bmsp_comm_unique_id.argtypes = [vp]
        L.bmsp_comm_init.argtypes = [vp, i, i, p(vp)]
        L.bmsp_comm_init_from_env.argtypes = [p(vp)]
        L.bmsp_comm_init_loopback.argtypes = [i, p(vp)]
        L.bmsp_shard_layout.argtypes = [i, vp, vp, vp, vp]
        L.bmsp_shard_row_slices.argtypes = [i, i, vp, vp, vp]
        L.bmsp_matrix_invalidate.argtypes = [vp, i]
        L.bmsp_comm_info.argtypes = [vp, p(i), p(i)]
        L.bmsp_comm_free.argtypes = [vp]
        L.bmsp_spgemm_sharded.argtypes = [vp, vp, vp, p(vp), i, i, i, vp, p(SpgemmStats), p(ShardStats)]
        L.bmsp_spgemm_sharded_ex.argtypes = [vp, vp, vp, p(vp), i, i, i, vp, p(SpgemmStats), p(ShardStats), i, i]
        L.bmsp_spmv_sharded.argtypes = [vp, vp, vp, vp, i, vp, p(ShardStats)]
        L.bmsp_csr_from_mtx.argtypes = [C.c_char_p, p(vp)]
        L.bmsp_csr_from_arrays.argtypes = [i, i, i64, vp, vp, vp, p(vp)]
        L.bmsp_csr_info.argtypes = [vp, p(i), p(i), p(i64)]
        L.bmsp_csr_arrays.argtypes = [vp, p(vp), p(vp), p(vp)]
        L.bmsp_csr_multiply.argtypes = [vp, vp, p(vp)]
        L.bmsp_csr_spmv.argtypes = [vp, vp, vp]
        L.bmsp_csr_multiply_host.argtypes = [vp, vp, p(vp), i]
        L.bmsp_csr_spmv_host.argtypes = [vp, vp, vp, i]
        L.bmsp_csr_free.argtypes = [vp]
        _lib = L
    return _lib


def check(status):
    if status != 0:
        raise BmspError(status, lib().bmsp_last_error().decode(errors="replace"))


# ---- device buffers ---------------------------------------------------------------------------------------
class DeviceArray:
    """a typed device buffer from the library's pool."""

    def __init__(self, n, dtype, ptr=None, owner=None):
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self._owned = ptr is None
        self._owner = owner  # keeps a parent (matrix) alive for borrowed pointers
        if ptr is None:
            q = C.c_void_p()
            check(lib().bmsp_malloc(C.byref(q), max(1, self.n) * self.dtype.itemsize))
            self.ptr = q.value
        else:
            self.ptr = int(ptr) if ptr else 0

    @staticmethod
    def from_host(arr, dtype=None):
        a = np.ascontiguousarray(arr, dtype=dtype)
        d = DeviceArray(a.size, a.dtype)
        if a.size:
            check(lib().bmsp_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes))
        return d

    def to_host(self):
        out = np.empty(self.n, dtype=self.dtype)
        if self.n:
            check(lib().bmsp_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def zero(self):
        if self.n:
            check(lib().bmsp_memset(self.ptr, 0, self.n * self.dtype.itemsize))

    def release(self):
        """gives the pointer away (ownership moves to a matrix that adopts it)."""
        self._owned = False
        return self.ptr

    def __del__(self):
        try:
            if self._owned and self.ptr:
                lib().bmsp_free(self.ptr)
        except Exception:
            pass


class Event:
    """hipEvent on the operators' stream (device-side timing)."""

    def __init__(self):
        e = C.c_void_p()
        check(lib().bmsp_event_create(C.byref(e)))
        self.e = e.value

    def record(self, stream=None):
        check(lib().bmsp_event_record(self.e, stream))

    def elapsed_ms(self, stop):
        ms = C.c_float()
        check(lib().bmsp_event_elapsed_ms(self.e, stop.e, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            lib().bmsp_event_destroy(self.e)
        except Exception:
            pass


def synchronize():
    check(lib().bmsp_synchronize())


def device_count():
    n = C.c_int()
    check(lib().bmsp_device_count(C.byref(n)))
    return n.value


def set_device(d):
    check(lib().bmsp_set_device(int(d)))


# ---- the container ------------------------------------------------------------------------------------------
class BmSpMatrix:
    """mirror of the reference's bmSpMatrix<T> (include/bmSpMatrix.h:20-40) over the C ABI."""

    def __init__(self, handle, parent=None):
        self.h = handle
        self._parent = parent

    # bmSpMatrix(std::string path, bool transpose)
    @staticmethod
    def from_mtx(path, transposed=False, dtype=F32):
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_mtx(os.fsencode(path), int(bool(transposed)), dtype, C.byref(h)))
        return BmSpMatrix(h.value)

    @staticmethod
    def from_coo(num_rows, num_cols, rows, cols, vals, transposed=False, dtype=F32):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert rows.shape == cols.shape == vals.shape
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_coo(int(num_rows), int(num_cols), rows.size, rows.ctypes.data, cols.ctypes.data,
                                         vals.ctypes.data, int(bool(transposed)), dtype, C.byref(h)))
        return BmSpMatrix(h.value)

    @staticmethod
    def from_coo_device(num_rows, num_cols, rows, cols, vals, transposed=False, dtype=F32, stream=None):
        """rows / cols int32, vals float64 DeviceArrays of equal length (bmsp_matrix_from_coo_device)."""
        assert rows.n == cols.n == vals.n
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_coo_device(int(num_rows), int(num_cols), rows.n, rows.ptr, cols.ptr, vals.ptr,
                                                int(bool(transposed)), dtype, stream, C.byref(h)))
        return BmSpMatrix(h.value)

    # bmSpMatrix(int num_rows, int num_cols, int block_num, keys&, bmps&, offsets&, values&)
    @staticmethod
    def from_arrays(num_rows, num_cols, keys, bmps, offsets, values, dtype=F32, transposed=False):
        """host arrays are copied to the device and adopted by the new matrix."""
        k = DeviceArray.from_host(keys, np.uint64)
        b = DeviceArray.from_host(bmps, np.uint64)
        o = DeviceArray.from_host(offsets, np.uint64)
        v = DeviceArray.from_host(values, NP_DTYPE[dtype])
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_arrays(int(num_rows), int(num_cols), k.n, v.n, k.ptr, b.ptr, o.ptr, v.ptr, dtype,
                                            int(bool(transposed)), 1, C.byref(h)))
        for d in (k, b, o, v):
            d.release()
        return BmSpMatrix(h.value)

    @staticmethod
    def from_device_arrays(num_rows, num_cols, keys, bmps, offsets, values, dtype=F32, transposed=False):
        """borrows DeviceArrays (ownership 2): `offsets` must hold block_num+1 entries; the arrays must outlive the matrix."""
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_arrays(int(num_rows), int(num_cols), keys.n, values.n, keys.ptr, bmps.ptr, offsets.ptr, values.ptr, dtype,
                                            int(bool(transposed)), 2, C.byref(h)))
        return BmSpMatrix(h.value, parent=(keys, bmps, offsets, values))

    def prepare(self, what=3, stream=None):
        """builds the cached sweep plan (1) / block-MAC operand records (2) ahead of the first product."""
        check(lib().bmsp_matrix_prepare(self.h, int(what), stream))
        return self

    def invalidate(self, structure_changed=False):
        """after writing the arrays in place: drops the cached derived structures (bmsp_matrix_invalidate)."""
        check(lib().bmsp_matrix_invalidate(self.h, int(bool(structure_changed))))
        return self

    def clone(self):
        """an independent device copy of the four arrays (bmsp_matrix_from_arrays, ownership 0)."""
        i = self.info()
        k, b, o, v = self.device_arrays()
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_arrays(i["num_rows"], i["num_cols"], i["block_num"], i["nnz"], k.ptr, b.ptr, o.ptr, v.ptr, i["dtype"],
                                            i["transposed"], 0, C.byref(h)))
        return BmSpMatrix(h.value)

    def save(self, path):
        check(lib().bmsp_matrix_save(self.h, os.fsencode(path)))

    @staticmethod
    def load(path):
        h = C.c_void_p()
        check(lib().bmsp_matrix_load(os.fsencode(path), C.byref(h)))
        return BmSpMatrix(h.value)

    def info(self):
        nr, nc, tr, dt = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nnz, nb = C.c_int64(), C.c_int64()
        check(lib().bmsp_matrix_info(self.h, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(nb), C.byref(dt), C.byref(tr)))
        return dict(num_rows=nr.value, num_cols=nc.value, nnz=nnz.value, block_num=nb.value, dtype=dt.value,
                    transposed=tr.value)

    num_rows = property(lambda s: s.info()["num_rows"])
    num_cols = property(lambda s: s.info()["num_cols"])
    nnz = property(lambda s: s.info()["nnz"])
    block_num = property(lambda s: s.info()["block_num"])
    dtype = property(lambda s: s.info()["dtype"])

    def device_arrays(self):
        """(keys, bmps, offsets, values) as borrowed DeviceArrays; offsets has block_num+1 entries."""
        k, b, o, v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().bmsp_matrix_arrays(self.h, C.byref(k), C.byref(b), C.byref(o), C.byref(v)))
        i = self.info()
        return (DeviceArray(i["block_num"], np.uint64, k.value or 0, self), DeviceArray(i["block_num"], np.uint64, b.value or 0, self),
                DeviceArray(i["block_num"] + 1, np.uint64, o.value or 0, self),
                DeviceArray(i["nnz"], NP_DTYPE[i["dtype"]], v.value or 0, self))

    def host_arrays(self):
        return tuple(a.to_host() for a in self.device_arrays())

    def block_row_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        check(lib().bmsp_matrix_block_row_ptr(self.h, C.byref(p), C.byref(n)))
        return DeviceArray(n.value + 1, np.uint32, p.value, self).to_host()

    def transpose(self, transposed=False, stream=None):
        """A^T as a new matrix with its tiles in layout `transposed` (bmsp_matrix_transpose): no COO round trip."""
        h = C.c_void_p()
        check(lib().bmsp_matrix_transpose(self.h, int(bool(transposed)), stream, C.byref(h)))
        return BmSpMatrix(h.value)

    def with_layout(self, transposed, stream=None):
        """this matrix with its tiles in layout `transposed` (bmsp_matrix_convert_layout; a copy when it already has it)."""
        h = C.c_void_p()
        check(lib().bmsp_matrix_convert_layout(self.h, int(bool(transposed)), stream, C.byref(h)))
        return BmSpMatrix(h.value)

    def prune(self, tol=0.0, rule="abs", keep_diagonal=False, transposed=None, stream=None):
        """(this matrix without the entries the rule drops, stats dict): pybmsp.prune"""
        return prune(self, tol, rule, keep_diagonal, transposed, stream)

    def tril(self, k=0, transposed=None, stream=None):
        """the stored entries with col - row <= k as a new matrix: pybmsp.tril"""
        return tril(self, k, transposed, stream)

    def triu(self, k=0, transposed=None, stream=None):
        """the stored entries with col - row >= k as a new matrix: pybmsp.triu"""
        return triu(self, k, transposed, stream)

    def band(self, lo=None, hi=None, complement=False, transposed=None, stream=None):
        """the stored entries with lo <= col - row <= hi (complement: the others) as a new matrix: pybmsp.select_band without the stats"""
        return select_band(self, lo, hi, complement, transposed, stream)[0]

    def mask(self, M, complement=False, transposed=None, stream=None):
        """the stored entries at the coordinates M stores (complement: does not store) as a new matrix: pybmsp.select_mask without the stats"""
        return select_mask(self, M, complement, transposed, stream)[0]

    def diagonal(self, stream=None):
        """the diagonal as a DeviceArray of min(num_rows, num_cols) entries, +0 where (i, i) is not stored: pybmsp.diagonal"""
        return diagonal(self, stream)

    def scale(self, left=None, right=None, div_left=False, div_right=False, transposed=None, stream=None):
        """diag(left) * this * diag(right) as a new matrix: pybmsp.scale"""
        return scale(self, left, right, div_left, div_right, transposed, stream)

    def scale_(self, left=None, right=None, div_left=False, div_right=False, stream=None):
        """the same into this matrix's own values (bmsp_matrix_scale_values with out == A)"""
        return scale_values(self, self, left, right, div_left, div_right, stream)

    @staticmethod
    def from_diagonal(d, num_rows=None, num_cols=None, dtype=F32, transposed=False, stream=None):
        """the matrix with d[i] stored at every (i, i): pybmsp.from_diagonal"""
        return from_diagonal(d, num_rows, num_cols, dtype, transposed, stream)

    def matvec(self, v, alpha=1.0, beta=0.0, u=None, stream=None):
        """alpha * this * v + beta * u, whatever the tile layout: pybmsp.spmv_op(op="N")"""
        return spmv_op(self, v, "N", alpha, beta, u, stream)

    def rmatvec(self, v, alpha=1.0, beta=0.0, u=None, stream=None):
        """alpha * this^T * v + beta * u without a transposed copy: pybmsp.spmv_op(op="T")"""
        return spmv_op(self, v, "T", alpha, beta, u, stream)

    def matmat(self, X, k, alpha=1.0, beta=0.0, Y=None, ldx=None, ldy=None, stream=None):
        """alpha * this * X + beta * Y for k vectors, whatever the tile layout: pybmsp.spmm_op(op="N")"""
        return spmm_op(self, X, k, "N", alpha, beta, Y, ldx, ldy, stream)

    def rmatmat(self, X, k, alpha=1.0, beta=0.0, Y=None, ldx=None, ldy=None, stream=None):
        """alpha * this^T * X + beta * Y for k vectors without a transposed copy: pybmsp.spmm_op(op="T")"""
        return spmm_op(self, X, k, "T", alpha, beta, Y, ldx, ldy, stream)

    def sddmm(self, X, Y, k, alpha=1.0, beta=0.0, mul_s=False, transposed=None, ldx=None, ldy=None, stream=None):
        """alpha * (X . Y^T) on this matrix's pattern (+ beta * this, or * this) as a new matrix: pybmsp.sddmm"""
        return sddmm(self, X, Y, k, alpha, beta, mul_s, transposed, ldx, ldy, stream)

    def sddmm_(self, X, Y, k, alpha=1.0, beta=0.0, mul_s=False, ldx=None, ldy=None, stream=None):
        """the same into this matrix's own values (bmsp_sddmm_values with out == S)"""
        return sddmm_values(self, self, X, Y, k, alpha, beta, mul_s, ldx, ldy, stream)

    def solve_triangular(self, b, op="N", fill="lower", unit_diag=False, alpha=1.0, x=None, stream=None):
        """x with op(tri(this)) * x = alpha * b: pybmsp.spsv"""
        return spsv(self, b, op, fill, unit_diag, alpha, x, stream)

    def solve_triangular_multi(self, B, k, op="N", fill="lower", unit_diag=False, alpha=1.0, X=None, ldb=None, ldx=None, stream=None):
        """X with op(tri(this)) * X = alpha * B for k right-hand sides: pybmsp.spsm"""
        return spsm(self, B, k, op, fill, unit_diag, alpha, X, ldb, ldx, stream)

    def solve_triangular_iterative(self, b, op="N", fill="lower", unit_diag=False, alpha=1.0, max_iter=0, tol=0.0, x=None, x0_given=False,
                                   history=False, stream=None):
        """block-Jacobi sweeps towards the x of op(tri(this)) * x = alpha * b: pybmsp.spitsv"""
        return spitsv(self, b, op, fill, unit_diag, alpha, max_iter, tol, x, x0_given, history, stream)

    def ilu0(self, max_iter=0, tol=0.0, out_transposed=None, history=False, stream=None):
        """(F, info[, history]): the incomplete factor ILU(0) of this matrix by fixed-point sweeps: pybmsp.ilu0"""
        return ilu0(self, max_iter, tol, out_transposed, history, stream)

    def fsai(self, S, op="N", scale="sqrt", transposed=None, pivot=False, stream=None):
        """(G, info[, pivot]): the factorised sparse approximate inverse of op(this) on S's lower-triangular pattern: pybmsp.fsai"""
        return fsai(self, S, op, scale, transposed, pivot, stream)

    def solve(self, b, method="cg", precond=None, op="N", max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
        """(x, info[, history]) with op(this) * x = b by CG or BiCGStab on the device: pybmsp.krylov_solve.  method "gmres" or
        "gmres(<m>)": restarted GMRES with restart 30 or m, pybmsp.gmres_solve (solve_gmres takes the restart as a keyword)"""
        restart = _gmres_restart(method)
        if restart is not None:
            return gmres_solve(self, b, precond, op, restart, max_iter, tol, x, x0_given, history, stream)
        return krylov_solve(self, b, method, precond, op, max_iter, tol, x, x0_given, history, stream)

    def solve_gmres(self, b, precond=None, op="N", restart=30, max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
        """(x, info[, history]) with op(this) * x = b by restarted GMRES on the device: pybmsp.gmres_solve"""
        return gmres_solve(self, b, precond, op, restart, max_iter, tol, x, x0_given, history, stream)

    def color_blocks(self, seed=0, stream=None):
        """(colors, perm, info): the greedy block colouring by hashed priorities and its ordering: pybmsp.color_blocks"""
        return color_blocks(self, seed, stream)

    def permute_blocks(self, row_perm=None, col_perm=None, transposed=None, stream=None):
        """P * this * Q^T at tile granularity as a new matrix: pybmsp.permute_blocks"""
        return permute_blocks(self, row_perm, col_perm, transposed, stream)

    def reorder_multicolor(self, seed=0, stream=None):
        """(B, perm, info): this matrix under the symmetric block permutation by its multi-colour ordering, B = P * this * P^T, whose
        triangular solves have info["colors"] levels (at most, with a trailing partial block-row); perm (new -> old) is what
        vec_permute_blocks takes"""
        _, perm, info = color_blocks(self, seed, stream)
        return permute_blocks(self, perm, perm, None, stream), perm, info

    def aggregate(self, seed=0, stream=None):
        """(agg, num_aggregates, info): the MIS(2) aggregates of this matrix's scalar graph: pybmsp.aggregate"""
        return aggregate(self, seed, stream)

    @staticmethod
    def from_aggregates(agg, num_aggregates, weights=None, num_rows=None, dtype=F32, transposed=False, stream=None):
        """the num_rows x num_aggregates matrix with weights[i] at (i, agg[i]): pybmsp.from_aggregates"""
        return from_aggregates(agg, num_aggregates, weights, num_rows, dtype, transposed, stream)

    def mult_masked(self, B, M, alpha=1.0, beta=0.0, mul_m=False, transposed=None, stream=None):
        """alpha * (this * B) on M's pattern (+ beta * M, or * M) as a new matrix: pybmsp.spgemm_masked"""
        return spgemm_masked(self, B, M, alpha, beta, mul_m, transposed, stream)

    def copy_values_from(self, src, stream=None):
        """re-gathers this matrix's values from `src`, which it was made from by transpose() / with_layout() (bmsp_matrix_copy_values)."""
        check(lib().bmsp_matrix_copy_values(src.h, self.h, stream))
        return self

    # generate_coo()
    def to_coo(self):
        n = self.nnz
        r, c, v = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
        check(lib().bmsp_matrix_to_coo_host(self.h, r.ctypes.data, c.ctypes.data, v.ctypes.data))
        return r, c, v

    def to_coo_device(self, stream=None):
        """(rows int32, cols int32, vals float64) DeviceArrays, sorted by (row, col)."""
        n = self.nnz
        r, c, v = DeviceArray(n, np.int32), DeviceArray(n, np.int32), DeviceArray(n, np.float64)
        check(lib().bmsp_matrix_to_coo_device(self.h, r.ptr, c.ptr, v.ptr, stream))
        return r, c, v

    def to_csr_device(self, stream=None):
        """(row_offsets int32 [num_rows+1], cols int32, vals float64) DeviceArrays."""
        i = self.info()
        ro, c, v = DeviceArray(i["num_rows"] + 1, np.int32), DeviceArray(i["nnz"], np.int32), DeviceArray(i["nnz"], np.float64)
        check(lib().bmsp_matrix_to_csr_device(self.h, ro.ptr, c.ptr, v.ptr, stream))
        return ro, c, v

    @staticmethod
    def from_csr_device(num_rows, num_cols, row_offsets, cols, vals, transposed=False, dtype=F32, stream=None):
        h = C.c_void_p()
        check(lib().bmsp_matrix_from_csr_device(int(num_rows), int(num_cols), cols.n, row_offsets.ptr, cols.ptr, vals.ptr,
                                                int(bool(transposed)), dtype, stream, C.byref(h)))
        return BmSpMatrix(h.value)

    # compare(coo)
    def compare(self, rows, cols, vals):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        err, miss = C.c_double(), C.c_int64()
        check(lib().bmsp_matrix_compare(self.h, rows.size, rows.ctypes.data, cols.ctypes.data, vals.ctypes.data,
                                        C.byref(err), C.byref(miss)))
        return err.value, miss.value

    def compare_device(self, rows, cols, vals, stream=None):
        """rows / cols int32, vals float64 DeviceArrays."""
        err, miss = C.c_double(), C.c_int64()
        check(lib().bmsp_matrix_compare_device(self.h, rows.n, rows.ptr, cols.ptr, vals.ptr, C.byref(err), C.byref(miss), stream))
        return err.value, miss.value

    def row_panel(self, brow_begin, brow_end):
        h = C.c_void_p()
        check(lib().bmsp_matrix_row_panel(self.h, int(brow_begin), int(brow_end), C.byref(h)))
        return BmSpMatrix(h.value, parent=self)

    def free(self):
        if self.h:
            lib().bmsp_matrix_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def add(A, B, alpha=1.0, beta=1.0, transposed=None, stream=None):
    """alpha*A + beta*B as a new matrix (bmsp_matrix_add), its tiles in layout `transposed` (None: A's layout)."""
    lay = A.info()["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    check(lib().bmsp_matrix_add(float(alpha), A.h, float(beta), B.h, lay, stream, C.byref(h)))
    return BmSpMatrix(h.value)


def add_values(Cm, A, B, alpha=1.0, beta=1.0, stream=None):
    """re-computes the values of Cm = add(A, B, ...) from A's and B's current values (bmsp_matrix_add_values)."""
    check(lib().bmsp_matrix_add_values(float(alpha), A.h, float(beta), B.h, Cm.h, stream))
    return Cm


def _prune_rule(rule):
    if rule not in _PRUNE_RULES:
        raise ValueError("rule must be 'abs' or 'row_rel' (got %r)" % (rule,))
    return _PRUNE_RULES[rule]


def prune(A, tol=0.0, rule="abs", keep_diagonal=False, transposed=None, stream=None):
    """A without the stored entries with |v| <= tol (rule "abs") or |v| <= tol * rowmax(row) (rule "row_rel") as a new matrix
    (bmsp_matrix_prune), its tiles in layout `transposed` (None: A's layout); returns (matrix, {"nnz_in", "nnz_out", "blocks_in",
    "blocks_out"}).  keep_diagonal: entries with row == col always stay."""
    lay = A.info()["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    st = PruneStats()
    check(lib().bmsp_matrix_prune(A.h, _prune_rule(rule), float(tol), PRUNE_KEEP_DIAGONAL if keep_diagonal else 0, lay, stream, C.byref(h),
                                  C.byref(st)))
    return BmSpMatrix(h.value), st.as_dict()


def prune_count(A, tol=0.0, rule="abs", keep_diagonal=False, stream=None):
    """the stats prune() would return, without making the output (the marking passes only)."""
    st = PruneStats()
    check(lib().bmsp_matrix_prune(A.h, _prune_rule(rule), float(tol), PRUNE_KEEP_DIAGONAL if keep_diagonal else 0, 0, stream, None, C.byref(st)))
    return st.as_dict()


def row_absmax(A, stream=None):
    """max |v| over the stored, non-NaN entries of every row (0 for a row with none) as a DeviceArray (float32; float64 for F64)."""
    i = A.info()
    out = DeviceArray(i["num_rows"], OUT_DTYPE[i["dtype"]])
    check(lib().bmsp_matrix_row_absmax(A.h, out.ptr, stream))
    return out


def _band_bounds(lo, hi):
    return BAND_MIN if lo is None else int(lo), BAND_MAX if hi is None else int(hi)


def select_band(A, lo=None, hi=None, complement=False, transposed=None, stream=None):
    """the stored entries (i, j) of A with lo <= j - i <= hi (None: unbounded on that side; complement: the entries outside the band) as a
    new matrix (bmsp_matrix_select_band), its tiles in layout `transposed` (None: A's layout); returns (matrix, {"nnz_in", "nnz_out",
    "blocks_in", "blocks_out"}).  No value is read; lo > hi is the empty band."""
    lo, hi = _band_bounds(lo, hi)
    lay = A.info()["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    st = SelectStats()
    check(lib().bmsp_matrix_select_band(A.h, lo, hi, SELECT_COMPLEMENT if complement else 0, lay, stream, C.byref(h), C.byref(st)))
    return BmSpMatrix(h.value), st.as_dict()


def band_count(A, lo=None, hi=None, complement=False, stream=None):
    """the stats select_band() would return, without making the output (the mark pass and the scan only)."""
    lo, hi = _band_bounds(lo, hi)
    st = SelectStats()
    check(lib().bmsp_matrix_select_band(A.h, lo, hi, SELECT_COMPLEMENT if complement else 0, 0, stream, None, C.byref(st)))
    return st.as_dict()


def tril(A, k=0, transposed=None, stream=None):
    """the stored entries of A with col - row <= k as a new matrix (numpy's tril on the stored pattern): select_band(A, None, k)"""
    return select_band(A, None, k, False, transposed, stream)[0]


def triu(A, k=0, transposed=None, stream=None):
    """the stored entries of A with col - row >= k as a new matrix (numpy's triu on the stored pattern): select_band(A, k, None)"""
    return select_band(A, k, None, False, transposed, stream)[0]


def offdiagonal(A, transposed=None, stream=None):
    """the stored entries of A with row != col as a new matrix (the off-diagonal part of a splitting): the complement of band(0, 0)"""
    return select_band(A, 0, 0, True, transposed, stream)[0]


def select_mask(A, M, complement=False, transposed=None, stream=None):
    """the stored entries of A at the coordinates M stores (complement: does not store) as a new matrix (bmsp_matrix_select_mask), its
    tiles in layout `transposed` (None: A's layout); returns (matrix, stats dict as select_band).  M has A's shape, any dtype and either
    layout; its values are never read."""
    lay = A.info()["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    st = SelectStats()
    check(lib().bmsp_matrix_select_mask(A.h, M.h, SELECT_COMPLEMENT if complement else 0, lay, stream, C.byref(h), C.byref(st)))
    return BmSpMatrix(h.value), st.as_dict()


def mask_count(A, M, complement=False, stream=None):
    """the stats select_mask() would return, without making the output."""
    st = SelectStats()
    check(lib().bmsp_matrix_select_mask(A.h, M.h, SELECT_COMPLEMENT if complement else 0, 0, stream, None, C.byref(st)))
    return st.as_dict()


def diagonal(A, stream=None):
    """the stored value at every (i, i), i < min(num_rows, num_cols), +0 where none is stored, as a DeviceArray (float32; float64 for
    F64) (bmsp_matrix_diagonal; asynchronous on `stream`)."""
    i = A.info()
    out = DeviceArray(min(i["num_rows"], i["num_cols"]), OUT_DTYPE[i["dtype"]])
    check(lib().bmsp_matrix_diagonal(A.h, out.ptr, stream))
    return out


def from_diagonal(d, num_rows=None, num_cols=None, dtype=F32, transposed=False, stream=None):
    """the num_rows x num_cols matrix (default: d.n x d.n) with d[i] stored at every (i, i), zeros included (bmsp_matrix_from_diagonal).
    d: DeviceArray of at least min(num_rows, num_cols) entries, float32 (float64 for F64)."""
    nr = d.n if num_rows is None else int(num_rows)
    nc = d.n if num_cols is None else int(num_cols)
    if d.dtype != np.dtype(OUT_DTYPE[dtype]) or d.n < min(nr, nc):
        raise ValueError("d must hold at least min(num_rows, num_cols) entries of %s" % np.dtype(OUT_DTYPE[dtype]).name)
    h = C.c_void_p()
    check(lib().bmsp_matrix_from_diagonal(nr, nc, d.ptr, dtype, int(bool(transposed)), stream, C.byref(h)))
    return BmSpMatrix(h.value)


def _scale_args(A, left, right, div_left, div_right):
    i = A.info()
    for name, v, n in (("left", left, i["num_rows"]), ("right", right, i["num_cols"])):
        if v is not None and (v.dtype != np.dtype(OUT_DTYPE[i["dtype"]]) or v.n < n):
            raise ValueError("%s must hold %d entries of %s" % (name, n, np.dtype(OUT_DTYPE[i["dtype"]]).name))
    flags = (SCALE_DIV_LEFT if div_left else 0) | (SCALE_DIV_RIGHT if div_right else 0)
    return i, None if left is None else left.ptr, None if right is None else right.ptr, flags


def scale(A, left=None, right=None, div_left=False, div_right=False, transposed=None, stream=None):
    """diag(left) * A * diag(right) as a new matrix with A's structure (bmsp_matrix_scale), its tiles in layout `transposed` (None: A's
    layout).  left / right: DeviceArrays of num_rows / num_cols entries (float32; float64 for F64); None skips that side; div_left /
    div_right divide by that side instead.  Asynchronous on `stream`."""
    i, lp, rp, flags = _scale_args(A, left, right, div_left, div_right)
    lay = i["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    check(lib().bmsp_matrix_scale(A.h, lp, rp, flags, lay, stream, C.byref(h)))
    return BmSpMatrix(h.value)


def scale_values(out, A, left=None, right=None, div_left=False, div_right=False, stream=None):
    """the values of diag(left) * A * diag(right) into `out`: A itself (in place) or a matrix made from A by scale() / with_layout()
    (bmsp_matrix_scale_values)."""
    _, lp, rp, flags = _scale_args(A, left, right, div_left, div_right)
    check(lib().bmsp_matrix_scale_values(A.h, lp, rp, flags, out.h, stream))
    return out


# bmSparse_SpMV(A, v, u, batched)
def spmv(A, v, u=None, batched=False, stream=None):
    """v: DeviceArray (A's dtype); returns u as a DeviceArray (float32, float64 for F64)."""
    i = A.info()
    if u is None:
        u = DeviceArray(i["num_rows"], OUT_DTYPE[i["dtype"]])
    check(lib().bmsp_spmv(A.h, v.ptr, u.ptr, SPMV_BATCHED if batched else SPMV_DEFAULT, stream))
    return u


def spmv_launch_info(A, variant=0):
    """{"kernel", "compulsory_bytes", "format_bytes"} of the launch bmsp_spmv would make for (A, variant)."""
    name = C.create_string_buffer(128)
    cb, fb = C.c_int64(), C.c_int64()
    check(lib().bmsp_spmv_launch_info(A.h, int(variant), name, 128, C.byref(cb), C.byref(fb)))
    return {"kernel": name.value.decode(), "compulsory_bytes": cb.value, "format_bytes": fb.value}


def _op(op):
    if op not in _OPS:
        raise ValueError("op must be 'N' or 'T' (got %r)" % (op,))
    return _OPS[op]


def spmv_op(A, v, op="N", alpha=1.0, beta=0.0, u=None, stream=None):
    """u = alpha * op(A) * v + beta * u (bmsp_spmv_op), op "N" or "T", A in either tile layout.  v: DeviceArray of A's dtype with num_cols
    ("N") / num_rows ("T") entries; u: DeviceArray (float32, float64 for F64) of the output length, made when None (beta must then be 0).
    Returns u.  Asynchronous on `stream` once the cached view of (A, op) exists."""
    o = _op(op)
    i = A.info()
    n_in, n_out = (i["num_rows"], i["num_cols"]) if o == OP_T else (i["num_cols"], i["num_rows"])
    if v.dtype != np.dtype(NP_DTYPE[i["dtype"]]) or v.n < n_in:
        raise ValueError("v must hold %d entries of %s" % (n_in, np.dtype(NP_DTYPE[i["dtype"]]).name))
    if u is None:
        if beta != 0:
            raise ValueError("beta != 0 needs u")
        u = DeviceArray(n_out, OUT_DTYPE[i["dtype"]])
    elif u.dtype != np.dtype(OUT_DTYPE[i["dtype"]]) or u.n < n_out:
        raise ValueError("u must hold %d entries of %s" % (n_out, np.dtype(OUT_DTYPE[i["dtype"]]).name))
    check(lib().bmsp_spmv_op(A.h, o, float(alpha), v.ptr, float(beta), u.ptr, stream))
    return u


def spmv_op_launch_info(A, op):
    """{"kernel", "slots", "items", "split_blocks", "view_bytes", "compulsory_bytes"} of the launch spmv_op(A, v, op) makes; builds the
    cached view of (A, op) if it is missing (bmsp_spmv_op_launch_info)."""
    o = _op(op)
    info = SpmvOpInfo()
    check(lib().bmsp_spmv_op_launch_info(A.h, o, C.byref(info)))
    return info.as_dict()


def spmv_op_plan_items(ptr, split):
    """(items [n, 4], folds [split blocks, 3], scratch slots) of the view's item planner for a block pointer (host arithmetic of
    spmv_op.hip; bmsp_spmv_op_plan_items)."""
    pt = np.ascontiguousarray(ptr, dtype=np.uint32)
    blocks = max(0, pt.size - 1)
    ni, nf, ns = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().bmsp_spmv_op_plan_items(pt.ctypes.data, blocks, int(split), None, None, C.byref(ni), C.byref(nf), C.byref(ns)))
    items, folds = np.zeros((ni.value, 4), np.uint32), np.zeros((nf.value, 3), np.uint32)
    check(lib().bmsp_spmv_op_plan_items(pt.ctypes.data, blocks, int(split), items.ctypes.data, folds.ctypes.data, C.byref(ni), C.byref(nf),
                                        C.byref(ns)))
    return items, folds, ns.value


def _fill(fill):
    if fill not in _FILLS:
        raise ValueError("fill must be 'lower' or 'upper' (got %r)" % (fill,))
    return _FILLS[fill]


def spsv(A, b, op="N", fill="lower", unit_diag=False, alpha=1.0, x=None, stream=None):
    """Solves op(tri(A)) * x = alpha * b on the device (bmsp_spsv): tri(A) the "lower" / "upper" triangle of the square A (named before
    op), op "N" or "T", A in either tile layout; unit_diag takes the diagonal as 1 and never reads the stored one.  b: DeviceArray of
    num_rows entries (float32, float64 for F64); x: the same, made when None, and may be b itself (in place).  Returns x.  One fused
    multiply-add per stored entry in the order of a sequential substitution, one IEEE division per row: the bits are fixed.  Asynchronous
    on `stream` once the plan of (A, op, fill) exists (spsv_analyse, or the first call)."""
    o, f = _op(op), _fill(fill)
    i = A.info()
    vt = np.dtype(OUT_DTYPE[i["dtype"]])
    if b.dtype != vt or b.n < i["num_rows"]:
        raise ValueError("b must hold %d entries of %s" % (i["num_rows"], vt.name))
    if x is None:
        x = DeviceArray(i["num_rows"], vt)
    elif x.dtype != vt or x.n < i["num_rows"]:
        raise ValueError("x must hold %d entries of %s" % (i["num_rows"], vt.name))
    check(lib().bmsp_spsv(A.h, o, f, DIAG_UNIT if unit_diag else DIAG_NON_UNIT, float(alpha), b.ptr, x.ptr, stream))
    return x


def spsv_analyse(A, op, fill, unit_diag=False, stream=None):
    """{"kernel", "levels", "max_level_width", "launches", "chain_launches", "chained_levels", "plan_bytes"} of the plan spsv(A, ., op,
    fill) runs; builds the plan if it is missing, which synchronises `stream` (bmsp_spsv_analyse)."""
    info = SpsvInfo()
    check(lib().bmsp_spsv_analyse(A.h, _op(op), _fill(fill), DIAG_UNIT if unit_diag else DIAG_NON_UNIT, stream, C.byref(info)))
    return info.as_dict()


def spsv_plan(ptr, other, lower, chain):
    """(level_of [blocks], order [blocks], level_ptr [levels + 1], segments [launches, 3]) of the solve's planner for a block pointer and
    the other-index column of its records (host arithmetic of spsv.hip; bmsp_spsv_plan)."""
    pt = np.ascontiguousarray(ptr, dtype=np.uint32)
    ot = np.ascontiguousarray(other, dtype=np.uint32)
    blocks = max(0, pt.size - 1)
    level_of, order = np.zeros(blocks, np.uint32), np.zeros(blocks, np.uint32)
    level_ptr, segments = np.zeros(blocks + 1, np.uint32), np.zeros((blocks, 3), np.uint32)
    nl, ns = C.c_int64(), C.c_int64()
    check(lib().bmsp_spsv_plan(pt.ctypes.data if pt.size else None, ot.ctypes.data if ot.size else None, blocks, int(bool(lower)), int(chain),
                               level_of.ctypes.data, order.ctypes.data, level_ptr.ctypes.data, segments.ctypes.data, C.byref(nl),
                               C.byref(ns)))
    return level_of, order, level_ptr[:nl.value + 1].copy(), segments[:ns.value].copy()


def spitsv(A, b, op="N", fill="lower", unit_diag=False, alpha=1.0, max_iter=0, tol=0.0, x=None, x0_given=False, history=False, stream=None):
    """Block-Jacobi sweeps towards the x of op(tri(A)) * x = alpha * b on the device (bmsp_spitsv); A, b, op, fill, unit_diag and alpha as
    for spsv.  A sweep is one launch: exact inside every 8 x 8 diagonal tile, the previous iterate between block-rows; after `levels`
    sweeps x holds spsv's bits.  Stops after a sweep that changed nothing or, with tol > 0, whose largest update is at most tol times the
    largest |x_i|; max_iter=0 means levels + 1.  tol=ITSV_NO_CHECK runs exactly max_iter sweeps asynchronously, nothing read back (history
    must be False).  x: DeviceArray for the result (made when None; never b); x0_given: x holds the initial iterate (default +0, x is not
    read).  Returns (x, info) or (x, info, history): info = {"kernel", "sweeps", "levels", "converged", "delta", "xmax"}, history = the
    delta of every sweep that ran (float64)."""
    o, f = _op(op), _fill(fill)
    i = A.info()
    vt = np.dtype(OUT_DTYPE[i["dtype"]])
    if b.dtype != vt or b.n < i["num_rows"]:
        raise ValueError("b must hold %d entries of %s" % (i["num_rows"], vt.name))
    if x is None:
        if x0_given:
            raise ValueError("x0_given needs x")
        x = DeviceArray(i["num_rows"], vt)
    elif x.dtype != vt or x.n < i["num_rows"]:
        raise ValueError("x must hold %d entries of %s" % (i["num_rows"], vt.name))
    info = SpitsvInfo()
    hist = None
    if history:
        cap = int(max_iter) if max_iter else spsv_analyse(A, op, fill, unit_diag, stream)["levels"] + 1
        hist = np.zeros(max(cap, 1), np.float64)
    check(lib().bmsp_spitsv(A.h, o, f, DIAG_UNIT if unit_diag else DIAG_NON_UNIT, float(alpha), b.ptr, x.ptr, int(max_iter), float(tol),
                            ITSV_X0_GIVEN if x0_given else 0, hist.ctypes.data if history else None, C.byref(info), stream))
    d = info.as_dict()
    return (x, d, hist[:d["sweeps"]].copy()) if history else (x, d)


def _ilu0_history(A, max_iter, history):
    if not history:
        return None
    cap = int(max_iter) if max_iter else 2 * A.info()["num_rows"]
    return np.zeros(max(cap, 1), np.float64)


def ilu0(A, max_iter=0, tol=0.0, out_transposed=None, history=False, stream=None):
    """The incomplete factorisation ILU(0) of A on its own pattern by fixed-point sweeps (bmsp_matrix_ilu0): F has A's structure in layout
    `out_transposed` (None: A's) and holds L (unit diagonal, not stored) below the diagonal and U on and above it -- what
    spsv(F, b, "N", "lower", True) followed by spsv(F, y, "N", "upper") applies.  A sweep is one launch that recomputes every stored entry
    from the previous iterate, started from A's values; after 2n - 1 sweeps F holds the sequential ILU(0) bit for bit.  Stops after a
    sweep that changed nothing or, with tol > 0, whose largest update is at most tol times the largest |f_ij|; max_iter=0 means 2n.
    tol=ILU_NO_CHECK runs exactly max_iter sweeps, nothing read back (history must be False).  A needs every diagonal entry stored.
    Returns (F, info) or (F, info, history): info = {"kernel", "lanes", "sweeps", "max_sweeps", "converged", "delta", "fmax",
    "view_bytes"}, history = the delta of every sweep that ran (float64)."""
    lay = A.info()["transposed"] if out_transposed is None else int(bool(out_transposed))
    info = Ilu0Info()
    hist = _ilu0_history(A, max_iter, history)
    h = C.c_void_p()
    check(lib().bmsp_matrix_ilu0(A.h, int(max_iter), float(tol), lay, stream, C.byref(h), hist.ctypes.data if history else None,
                                 C.byref(info)))
    d = info.as_dict()
    F = BmSpMatrix(h.value)
    return (F, d, hist[:d["sweeps"]].copy()) if history else (F, d)


def ilu0_values(A, F, max_iter=0, tol=0.0, history=False, stream=None, f0_given=False):
    """the sweeps of ilu0(A, ...) into an existing F made from A by ilu0() / with_layout() / scale() / sddmm() / spgemm_masked(); never A
    itself.  f0_given: start from F's current values, the warm start after a value-only update of A (default: from A's values, F is not
    read).  Returns (F, info) or (F, info, history) (bmsp_matrix_ilu0_values)."""
    if F is A or (F.h is not None and F.h == A.h):
        raise ValueError("F must not be A: a is read in every sweep")
    info = Ilu0Info()
    hist = _ilu0_history(A, max_iter, history)
    check(lib().bmsp_matrix_ilu0_values(A.h, F.h, int(max_iter), float(tol), ILU_F0_GIVEN if f0_given else 0, stream,
                                        hist.ctypes.data if history else None, C.byref(info)))
    d = info.as_dict()
    return (F, d, hist[:d["sweeps"]].copy()) if history else (F, d)


def _vec_f64(x, y):
    if x.dtype != y.dtype or x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("x and y must both be float32 or both float64 (got %s, %s)" % (x.dtype.name, y.dtype.name))
    return 1 if x.dtype == np.dtype(np.float64) else 0


def vec_dot(x, y, n=None, out=None, stream=None):
    """sum_i x_i * y_i over the first n entries (default: all of x) of two float32 or two float64 DeviceArrays as a float64 in device
    memory (bmsp_vec_dot): accumulated in double in the fixed tree include/bmsp.h writes out, so the result is a pure function of x, y and
    n.  Asynchronous on `stream`.  Returns `out`, a float64 DeviceArray of one entry (made when None)."""
    f64 = _vec_f64(x, y)
    n = x.n if n is None else int(n)
    if n > x.n or n > y.n:
        raise ValueError("n = %d exceeds the arrays (%d, %d)" % (n, x.n, y.n))
    if out is None:
        out = DeviceArray(1, np.float64)
    elif out.dtype != np.dtype(np.float64) or out.n < 1:
        raise ValueError("out must hold one float64")
    check(lib().bmsp_vec_dot(n, f64, x.ptr, y.ptr, out.ptr, stream))
    return out


def vec_axpby(a, x, b, y, n=None, stream=None):
    """y = fl(fl(a * x) + fl(b * y)) over the first n entries (default: all of x), a and b rounded once to the vectors' type, every
    operation rounded on its own; with b == 0 y is not read (bmsp_vec_axpby).  Asynchronous on `stream`.  Returns y."""
    f64 = _vec_f64(x, y)
    n = x.n if n is None else int(n)
    if n > x.n or n > y.n:
        raise ValueError("n = %d exceeds the arrays (%d, %d)" % (n, x.n, y.n))
    check(lib().bmsp_vec_axpby(n, f64, float(a), x.ptr, float(b), y.ptr, stream))
    return y


def color_blocks(A, seed=0, stream=None, want_perm=True):
    """(colors, perm, info) of the greedy colouring of A's block-row graph by hashed priorities (bmsp_matrix_color_blocks): A square, any
    dtype, either layout; block-rows I != J are neighbours iff a tile (I, J) or (J, I) is stored.  colors: uint32 DeviceArray of
    ceil(n / 8) entries, a pure function of structure and seed; perm (new -> old; None with want_perm=False): the block-rows sorted by
    (colour class, index), a trailing partial block-row kept last -- permute_blocks(A, perm, perm) has triangles of at most
    info["colors"] levels.  info = {"kernel", "blocks", "colors", "rounds", "view_bytes"}.  Synchronises `stream`."""
    nb = (A.info()["num_rows"] + 7) // 8
    colors = DeviceArray(nb, np.uint32)
    perm = DeviceArray(nb, np.uint32) if want_perm else None
    info = ColorInfo()
    check(lib().bmsp_matrix_color_blocks(A.h, int(seed) & 0xFFFFFFFFFFFFFFFF, colors.ptr, perm.ptr if want_perm else None, stream,
                                         C.byref(info)))
    return colors, perm, info.as_dict()


def _block_perm(perm, blocks, name):
    if perm is None:
        return None
    if perm.dtype != np.dtype(np.uint32) or perm.n < blocks:
        raise ValueError("%s must hold %d entries of uint32" % (name, blocks))
    return perm.ptr


def permute_blocks(A, row_perm=None, col_perm=None, transposed=None, stream=None):
    """P * A * Q^T at tile granularity as a new matrix with its tiles in layout `transposed` (None: A's): block (I', J') is block
    (row_perm[I'], col_perm[J']) of A, the gather convention A[p][:, q] (bmsp_matrix_permute_blocks).  row_perm / col_perm: uint32
    DeviceArrays of ceil(num_rows / 8) / ceil(num_cols / 8) entries, None = the identity; each is checked on the device to be a
    permutation that keeps a trailing partial block in place.  Whole tiles move, values as raw bits; copy_values_from(A) replays a
    value-only update of A.  Synchronises `stream`."""
    i = A.info()
    lay = i["transposed"] if transposed is None else int(transposed)
    h = C.c_void_p()
    check(lib().bmsp_matrix_permute_blocks(A.h, _block_perm(row_perm, (i["num_rows"] + 7) // 8, "row_perm"),
                                           _block_perm(col_perm, (i["num_cols"] + 7) // 8, "col_perm"), lay, stream, C.byref(h)))
    return BmSpMatrix(h.value)


def vec_permute_blocks(perm, x, inverse=False, y=None, n=None, stream=None):
    """The block permutation of a float32 / float64 DeviceArray of n entries (default: all of x) by perm, a uint32 DeviceArray of
    ceil(n / 8) entries (bmsp_vec_permute_blocks): y[8 i + r] = x[8 perm[i] + r] (b' = P b), or with inverse=True
    y[8 perm[i] + r] = x[8 i + r] (x = P^T x').  y: made when None (zeroed), never x.  An entry of perm out of range is skipped.
    Asynchronous on `stream`.  Returns y."""
    n = x.n if n is None else int(n)
    if y is None:
        y = DeviceArray(n, x.dtype)
        y.zero()
    f64 = _vec_f64(x, y)
    if n > x.n or n > y.n:
        raise ValueError("n = %d exceeds the arrays (%d, %d)" % (n, x.n, y.n))
    if perm.dtype != np.dtype(np.uint32) or perm.n < (n + 7) // 8:
        raise ValueError("perm must hold %d entries of uint32" % ((n + 7) // 8))
    check(lib().bmsp_vec_permute_blocks(n, f64, perm.ptr, int(inverse), x.ptr, y.ptr, stream))
    return y


def aggregate(S, seed=0, stream=None):
    """(agg, num_aggregates, info) of the MIS(2) aggregation of the scalar graph of a square S (bmsp_matrix_aggregate): any dtype, either
    layout, structure only; rows i != j are neighbours iff (i, j) or (j, i) is stored.  agg: uint32 DeviceArray of num_rows entries, every
    entry below num_aggregates, a pure function of structure and seed.  info = {"kernel", "nodes", "aggregates", "rounds", "launches",
    "view_bytes"}.  Synchronises `stream`."""
    agg = DeviceArray(S.info()["num_rows"], np.uint32)
    count = C.c_int64()
    info = AggregateInfo()
    check(lib().bmsp_matrix_aggregate(S.h, int(seed) & 0xFFFFFFFFFFFFFFFF, agg.ptr, C.byref(count), stream, C.byref(info)))
    return agg, count.value, info.as_dict()


def from_aggregates(agg, num_aggregates, weights=None, num_rows=None, dtype=F32, transposed=False, stream=None):
    """the num_rows x num_aggregates matrix (default: agg.n rows) with weights[i] (None: 1) stored at (i, agg[i]), one entry per row, its
    tiles in layout `transposed` (bmsp_matrix_from_aggregates).  agg: uint32 DeviceArray, an entry 0xFFFFFFFF leaves its row empty, any
    other entry must be below num_aggregates (checked on the device); weights: DeviceArray of float32 (float64 for F64).  Equals
    from_coo_device on the same triples bit for bit.  Synchronises `stream`."""
    nr = agg.n if num_rows is None else int(num_rows)
    if agg.dtype != np.dtype(np.uint32) or agg.n < nr:
        raise ValueError("agg must hold %d entries of uint32" % nr)
    if weights is not None and (weights.dtype != np.dtype(OUT_DTYPE[dtype]) or weights.n < nr):
        raise ValueError("weights must hold %d entries of %s" % (nr, np.dtype(OUT_DTYPE[dtype]).name))
    h = C.c_void_p()
    check(lib().bmsp_matrix_from_aggregates(nr, int(num_aggregates), agg.ptr, None if weights is None else weights.ptr, dtype,
                                            int(bool(transposed)), stream, C.byref(h)))
    return BmSpMatrix(h.value)


def _precond(precond):
    """None | "jacobi" | ("ilu", F) | ("ilu_sweeps", F, m) -> (Precond or None, the F to keep alive)"""
    if precond is None or precond == "none":
        return None, None
    if precond == "jacobi":
        return Precond(PC_JACOBI, None, 0), None
    if isinstance(precond, Precond):
        return precond, None
    if isinstance(precond, (tuple, list)) and len(precond) == 2 and precond[0] == "ilu":
        return Precond(PC_ILU_EXACT, precond[1].h, 0), precond[1]
    if isinstance(precond, (tuple, list)) and len(precond) == 3 and precond[0] == "ilu_sweeps":
        return Precond(PC_ILU_SWEEPS, precond[1].h, int(precond[2])), precond[1]
    raise ValueError("precond must be None, 'jacobi', ('ilu', F) or ('ilu_sweeps', F, m) (got %r)" % (precond,))


def krylov_solve(A, b, method="cg", precond=None, op="N", max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
    """Solves op(A) * x = b on the device by preconditioned CG (method "cg", A symmetric positive definite) or BiCGStab ("bicgstab"), A
    square, F32 or F64, in either tile layout (bmsp_krylov_solve).  precond: None, "jacobi", ("ilu", F) -- F from ilu0(), applied by two
    spsv -- or ("ilu_sweeps", F, m) -- the same two solves by m spitsv sweeps each.  Stops when dot(r, r) <= tol^2 * dot(b, b), after
    max_iter iterations (0: min(n, 2^20)) or on a breakdown; tol=KRYLOV_NO_CHECK runs exactly max_iter iterations asynchronously, nothing
    read back (history must be False).  x: DeviceArray for the result (made when None; never b); x0_given: x holds the initial iterate
    (default +0, x is not read).  The whole iteration is enqueued on `stream`; the scalars stay on the device.  Returns (x, info) or (x,
    info, history): info = {"method", "iterations", "max_iterations", "status" (KRYLOV_MAXITER / _CONVERGED / _BREAKDOWN), "relres",
    "bnorm", "products", "precond_applies", "workspace_bytes"}, history = the relative residual of every iteration (float64)."""
    if method not in _METHODS:
        raise ValueError("method must be 'cg' or 'bicgstab' (got %r)" % (method,))
    pc, keep = _precond(precond)  # (keep: the factor lives until the call has returned)
    i = A.info()
    return _solve_call(i["num_rows"], np.dtype(OUT_DTYPE[i["dtype"]]), b, x, x0_given, max_iter, tol, history, stream,
                       lambda *tail: lib().bmsp_krylov_solve(A.h, _op(op), _METHODS[method], C.byref(pc) if pc is not None else None, *tail))


def _gmres_restart(method):
    """"gmres" -> 30, "gmres(<m>)" -> m, anything else -> None"""
    if method == "gmres":
        return 30
    if isinstance(method, str) and method.startswith("gmres(") and method.endswith(")") and method[6:-1].isdigit():
        return int(method[6:-1])
    return None


def _solve_vectors(n, vt, b, x, x0_given, max_iter, history):
    """the checks of a solve's vectors; returns (x, the history buffer or None)"""
    if b.dtype != vt or b.n < n:
        raise ValueError("b must hold %d entries of %s" % (n, vt.name))
    if x is None:
        if x0_given:
            raise ValueError("x0_given needs x")
        x = DeviceArray(n, vt)
    elif x.dtype != vt or x.n < n:
        raise ValueError("x must hold %d entries of %s" % (n, vt.name))
    hist = None
    if history:
        cap = int(max_iter) if max_iter else min(n, 1 << 20)
        hist = np.zeros(max(cap, 1), np.float64)
    return x, hist


def _solve_call(n, vt, b, x, x0_given, max_iter, tol, history, stream, call):
    """the tail every solve shares: the vector checks, then call(d_b, d_x, max_iter, tol, flags, relres_history, info, stream) -- the
    arguments every bmsp_*_solve* ends with -- and (x, info) or (x, info, history) from what it left"""
    x, hist = _solve_vectors(n, vt, b, x, x0_given, max_iter, history)
    info = KrylovInfo()
    check(call(b.ptr, x.ptr, int(max_iter), float(tol), KRYLOV_X0_GIVEN if x0_given else 0, hist.ctypes.data if history else None,
               C.byref(info), stream))
    d = info.as_dict()
    return (x, d, hist[:d["iterations"]].copy()) if history else (x, d)


def gmres_solve(A, b, precond=None, op="N", restart=30, max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
    """Solves op(A) * x = b on the device by restarted GMRES (bmsp_gmres_solve): right-preconditioned GMRES(restart), restart 1 .. 256
    (0: 30), the basis orthogonalised by classical Gram-Schmidt applied twice.  One product and one preconditioner application per
    iteration, plus one product per restart.  Everything else -- A, b, precond, op, max_iter, tol, KRYLOV_NO_CHECK, x, x0_given, history,
    stream and the results -- is krylov_solve's; info["method"] is "gmres(<m>)+<preconditioner>"."""
    pc, keep = _precond(precond)  # (keep: the factor lives until the call has returned)
    i = A.info()
    return _solve_call(i["num_rows"], np.dtype(OUT_DTYPE[i["dtype"]]), b, x, x0_given, max_iter, tol, history, stream,
                       lambda *tail: lib().bmsp_gmres_solve(A.h, _op(op), C.byref(pc) if pc is not None else None, int(restart), *tail))


class Multigrid:
    """The V-cycle of a hierarchy on the device (bmsp_mg_create): A a list of `levels` square BmSpMatrix (F32 or F64, one dtype), P a list
    of levels - 1 prolongators (n_l x n_{l+1}), R None (restrict by P^T) or a list of restrictions / None entries, coarse_inv None or the
    dense inverse of A[-1] (numpy array or DeviceArray, row-major; ld_inv its leading dimension when it is not n_c), omega the damping
    of the Jacobi steps, pre / post their numbers.  Any operator in either tile layout.  The object keeps the operators alive; the
    library copies the diagonals and the inverse at construction, so new values of A mean a new Multigrid.  CG needs a symmetric
    cycle: R = P^T and pre == post."""

    def __init__(self, A, P, R=None, coarse_inv=None, omega=2.0 / 3.0, pre=1, post=1, ld_inv=None, stream=None):
        A, P = list(A), list(P)
        R = None if R is None else list(R)
        levels = len(A)
        if len(P) != max(levels - 1, 0) or (R is not None and len(R) != len(P)):
            raise ValueError("P (and R) must hold len(A) - 1 operators")
        self._keep = (A, P, R)
        self.h = None
        vt = np.dtype(OUT_DTYPE[A[0].info()["dtype"]]) if levels else np.dtype(np.float32)
        self.dtype, self.n = vt, (A[0].info()["num_rows"] if levels else 0)
        handles = lambda ms: (C.c_void_p * max(len(ms), 1))(*[None if m is None else m.h for m in ms])
        inv = coarse_inv
        if inv is not None and not isinstance(inv, DeviceArray):
            a = np.ascontiguousarray(inv, vt)
            if ld_inv is None:
                ld_inv = a.shape[1] if a.ndim == 2 else A[-1].info()["num_rows"]
            inv = DeviceArray.from_host(a.ravel())
        if ld_inv is None:
            ld_inv = A[-1].info()["num_rows"] if levels else 0
        h = C.c_void_p()
        check(lib().bmsp_mg_create(levels, handles(A), handles(P), None if R is None else handles(R), None if inv is None else inv.ptr,
                                   int(ld_inv), float(omega), int(pre), int(post), stream, C.byref(h)))
        self.h = h.value

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.bmsp_mg_free(self.h)
            self.h = None

    def info(self):
        i = MgInfo()
        check(lib().bmsp_mg_info(self.h, C.byref(i)))
        return i.as_dict()

    def vcycle(self, r, z=None, stream=None):
        """z = one cycle for right-hand side r from z = 0 (DeviceArrays of the vector type; z is made when None), asynchronous on `stream`"""
        if r.dtype != self.dtype or r.n < self.n:
            raise ValueError("r must hold %d entries of %s" % (self.n, self.dtype.name))
        if z is None:
            z = DeviceArray(self.n, self.dtype)
        elif z.dtype != self.dtype or z.n < self.n:
            raise ValueError("z must hold %d entries of %s" % (self.n, self.dtype.name))
        check(lib().bmsp_mg_vcycle(self.h, r.ptr, z.ptr, stream))
        return z

    def solve(self, b, method="cg", max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None, restart=30):
        """A[0] * x = b by CG or BiCGStab preconditioned by one cycle (bmsp_mg_solve): krylov_solve's arguments and results.  method
        "gmres": GMRES(restart) preconditioned by one cycle (bmsp_mg_solve_gmres), which takes any cycle"""
        if method == "gmres":
            return _solve_call(self.n, self.dtype, b, x, x0_given, max_iter, tol, history, stream,
                               lambda *tail: lib().bmsp_mg_solve_gmres(self.h, int(restart), *tail))
        if method not in _METHODS:
            raise ValueError("method must be 'cg', 'bicgstab' or 'gmres' (got %r)" % (method,))
        return _solve_call(self.n, self.dtype, b, x, x0_given, max_iter, tol, history, stream,
                           lambda *tail: lib().bmsp_mg_solve(self.h, _METHODS[method], *tail))


def fsai(A, S, op="N", scale="sqrt", transposed=None, pivot=False, stream=None):
    """The factorised sparse approximate inverse of op(A) on the pattern of S (bmsp_matrix_fsai): row i of G solves the small dense system
    on the stored columns of row i of S -- S lower triangular with the diagonal stored, at most 64 entries per row, values ignored -- and
    is scaled by `scale`: "none" (g = y), "sqrt" (g = y / sqrt(y_m): G A G^T has a unit diagonal) or "unit" (g = y / y_m).  G has S's
    structure, A's dtype (F32 or F64) and its tiles in layout `transposed` (None: S's layout).  Returns (G, info) or, with pivot=True,
    (G, info, pivot): the DeviceArray of the n values y_m; info = {"kernel", "lanes", "rows", "max_row", "pairs", "bad_rows",
    "lds_bytes"}.  Synchronises `stream`."""
    lay = S.info()["transposed"] if transposed is None else int(bool(transposed))
    i = A.info()
    d = DeviceArray(i["num_rows"], OUT_DTYPE[i["dtype"]]) if pivot else None
    h, info = C.c_void_p(), FsaiInfo()
    check(lib().bmsp_matrix_fsai(A.h, _op(op), S.h, _FSAI_SCALES[scale], lay, d.ptr if pivot else None, stream, C.byref(h), C.byref(info)))
    G = BmSpMatrix(h.value)
    return (G, info.as_dict(), d) if pivot else (G, info.as_dict())


def fsai_values(A, G, op="N", scale="sqrt", pivot=False, stream=None):
    """fsai(A, ...)'s values into an existing G -- made by fsai(), or any matrix of A's shape and dtype with a legal pattern -- after A's
    values changed (bmsp_matrix_fsai_values).  Returns (G, info) or (G, info, pivot).  Synchronises `stream`."""
    i = A.info()
    d = DeviceArray(i["num_rows"], OUT_DTYPE[i["dtype"]]) if pivot else None
    info = FsaiInfo()
    check(lib().bmsp_matrix_fsai_values(A.h, _op(op), G.h, _FSAI_SCALES[scale], d.ptr if pivot else None, stream, C.byref(info)))
    return (G, info.as_dict(), d) if pivot else (G, info.as_dict())


def fsai_pattern(A, theta=0.0, transposed=None, stream=None):
    """A pattern for fsai(): the lower triangle of A's pattern, after prune(theta, "row_rel", keep_diagonal=True) when theta > 0 (tiles in
    layout `transposed`; None: A's layout).  Both steps run on the device (bmsp_matrix_prune, bmsp_matrix_select_band)."""
    lay = A.info()["transposed"] if transposed is None else int(bool(transposed))
    M = prune(A, float(theta), "row_rel", True, None, stream)[0] if theta > 0 else A
    return tril(M, 0, lay, stream)


class Fsai:
    """The FSAI preconditioner of A on the pattern S (bmsp_fsai_create): kind "spd" -- G = fsai(A, N, S, sqrt), z = G^T (G r), symmetric
    positive definite, so CG may use it -- or "general" -- z = W^T (L r) with L = fsai(A, N, S, none), W = fsai(A, T, S, unit).  The
    application is two spmv_op calls; materialise=False applies the second as op T instead of on a materialised transpose, colmajor=True
    puts every factor in the column-major layout.  The object keeps A alive; S may go after construction."""

    def __init__(self, A, S, kind="spd", materialise=True, colmajor=False, stream=None):
        self.h = None
        self._keep = A
        i = A.info()
        self.dtype, self.n = np.dtype(OUT_DTYPE[i["dtype"]]), i["num_rows"]
        flags = (0 if materialise else FSAI_NO_MATERIALISE) | (FSAI_COLMAJOR if colmajor else 0)
        h = C.c_void_p()
        check(lib().bmsp_fsai_create(A.h, S.h, _FSAI_KINDS[kind], flags, stream, C.byref(h)))
        self.h = h.value

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.bmsp_fsai_free(self.h)
            self.h = None

    def info(self):
        i = FsaiHandleInfo()
        check(lib().bmsp_fsai_get_info(self.h, C.byref(i)))
        return i.as_dict()

    def factors(self):
        """(G1, G2): the two factors as borrowed BmSpMatrix (G2 is G1 for kind "spd"); they live as long as this object"""
        a, b = C.c_void_p(), C.c_void_p()
        check(lib().bmsp_fsai_factors(self.h, C.byref(a), C.byref(b)))
        out = []
        for q in (a, b):
            m = BmSpMatrix(q.value, parent=self)
            m.free = lambda: None  # (lent: the handle frees it)
            out.append(m)
        return tuple(out)

    def update(self, stream=None):
        """new factor values after a value update of A (bmsp_fsai_update)"""
        check(lib().bmsp_fsai_update(self.h, stream))
        return self

    def apply(self, r, z=None, stream=None):
        """z = G2^T (G1 r) (DeviceArrays of the vector type; z is made when None), asynchronous on `stream`"""
        if r.dtype != self.dtype or r.n < self.n:
            raise ValueError("r must hold %d entries of %s" % (self.n, self.dtype.name))
        if z is None:
            z = DeviceArray(self.n, self.dtype)
        elif z.dtype != self.dtype or z.n < self.n:
            raise ValueError("z must hold %d entries of %s" % (self.n, self.dtype.name))
        check(lib().bmsp_fsai_apply(self.h, r.ptr, z.ptr, stream))
        return z

    def solve(self, b, method="cg", max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
        """A x = b by CG or BiCGStab preconditioned by this (bmsp_fsai_solve): krylov_solve's arguments and results; method "gmres" or
        "gmres(<m>)" goes to solve_gmres"""
        restart = _gmres_restart(method)
        if restart is not None:
            return self.solve_gmres(b, restart, max_iter, tol, x, x0_given, history, stream)
        if method not in _METHODS:
            raise ValueError("method must be 'cg', 'bicgstab' or 'gmres' (got %r)" % (method,))
        return _solve_call(self.n, self.dtype, b, x, x0_given, max_iter, tol, history, stream,
                           lambda *tail: lib().bmsp_fsai_solve(self.h, _METHODS[method], *tail))

    def solve_gmres(self, b, restart=30, max_iter=0, tol=1e-6, x=None, x0_given=False, history=False, stream=None):
        """A x = b by GMRES(restart) preconditioned by this (bmsp_fsai_solve_gmres): gmres_solve's arguments and results"""
        return _solve_call(self.n, self.dtype, b, x, x0_given, max_iter, tol, history, stream,
                           lambda *tail: lib().bmsp_fsai_solve_gmres(self.h, int(restart), *tail))


def _spsm_strides(k, ldb, ldx):
    k = int(k)
    ldb = k if ldb is None else int(ldb)
    ldx = k if ldx is None else int(ldx)
    if k < 1:
        raise ValueError("k must be >= 1 (got %d)" % k)
    if ldb < k or ldx < k:
        raise ValueError("ldb and ldx must be >= k (got ldb = %d, ldx = %d, k = %d)" % (ldb, ldx, k))
    return k, ldb, ldx


def spsm(A, B, k, op="N", fill="lower", unit_diag=False, alpha=1.0, X=None, ldb=None, ldx=None, stream=None):
    """Solves op(tri(A)) * X = alpha * B for k right-hand sides on the device (bmsp_spsm); op, fill and unit_diag as for spsv.  B:
    DeviceArray (float32, float64 for F64), row-major num_rows x k at leading dimension ldb (default k); X: the same at leading dimension
    ldx (default k), made as num_rows x ldx when None, and may be B itself (in place: ldx must then equal ldb).  Returns X.  Column c of X
    holds the bits spsv writes for column c of B; one walk of the dependency chain carries all k columns.  Asynchronous on `stream` once
    the plan of (A, op, fill) exists (spsv_analyse, spsm_launch_info, or the first solve)."""
    o, f = _op(op), _fill(fill)
    k, ldb, ldx = _spsm_strides(k, ldb, ldx)
    i = A.info()
    n = i["num_rows"]
    vt = np.dtype(OUT_DTYPE[i["dtype"]])
    need_b = (n - 1) * ldb + k if n else 0
    if B.dtype != vt or B.n < need_b:
        raise ValueError("B must hold %d entries of %s" % (need_b, vt.name))
    if X is None:
        X = DeviceArray(n * ldx, vt)
    else:
        need_x = (n - 1) * ldx + k if n else 0
        if X.dtype != vt or X.n < need_x:
            raise ValueError("X must hold %d entries of %s" % (need_x, vt.name))
        if X is B and ldx != ldb:
            raise ValueError("in place (X is B) needs ldx == ldb (got ldb = %d, ldx = %d)" % (ldb, ldx))
    check(lib().bmsp_spsm(A.h, o, f, DIAG_UNIT if unit_diag else DIAG_NON_UNIT, float(alpha), B.ptr, ldb, X.ptr, ldx, k, stream))
    return X


def spsm_launch_info(A, op, fill, k, unit_diag=False, ldb=None, ldx=None, stream=None):
    """{"kernel", "lanes", "col_chunks", "levels", "launches", "chain_launches", "chained_levels", "plan_bytes"} of the launches spsm(A, B,
    k, op, fill) makes; builds the plan of (A, op, fill) if it is missing, which synchronises `stream` (bmsp_spsm_launch_info)."""
    o, f = _op(op), _fill(fill)
    k, ldb, ldx = _spsm_strides(k, ldb, ldx)
    info = SpsmInfo()
    check(lib().bmsp_spsm_launch_info(A.h, o, f, DIAG_UNIT if unit_diag else DIAG_NON_UNIT, k, ldb, ldx, stream, C.byref(info)))
    return info.as_dict()


def spmv_chunk_layout(A):
    """layout of the chunked sweep's cache for A: 0 = the sweep does not take spmv_chunk_kernel, 1 = storage order, 2 = row-sorted."""
    out = C.c_int()
    check(lib().bmsp_spmv_chunk_layout(A.h, C.byref(out)))
    return out.value


def spmm(A, X, k, Y=None, ldx=None, ldy=None, stream=None):
    """X: DeviceArray holding num_cols x k row-major (A's dtype); returns Y (num_rows x k, float32 / float64 for F64)."""
    i = A.info()
    ldx = k if ldx is None else ldx
    ldy = k if ldy is None else ldy
    if Y is None:
        Y = DeviceArray(i["num_rows"] * ldy, OUT_DTYPE[i["dtype"]])
    check(lib().bmsp_spmm(A.h, X.ptr, int(ldx), Y.ptr, int(ldy), int(k), stream))
    return Y


def spmm_launch_info(A, k, ldx=None, ldy=None):
    """the name of the kernel spmm(A, X, k, ldx=ldx, ldy=ldy) launches (bmsp_spmm_launch_info; "spmv: ..." when handed to the SpMV)."""
    name = C.create_string_buffer(160)
    check(lib().bmsp_spmm_launch_info(A.h, int(k), int(k if ldx is None else ldx), int(k if ldy is None else ldy), name, 160))
    return name.value.decode()


def spmm_op(A, X, k, op="N", alpha=1.0, beta=0.0, Y=None, ldx=None, ldy=None, stream=None):
    """Y = alpha * op(A) * X + beta * Y for k vectors (bmsp_spmm_op), op "N" or "T", A in either tile layout.  X: DeviceArray of A's dtype,
    row-major num_cols ("N") / num_rows ("T") x k at leading dimension ldx (default k); Y: DeviceArray (float32, float64 for F64), row-major
    output length x k at leading dimension ldy (default k), made when None (beta must then be 0).  Returns Y.  Asynchronous on `stream`
    once the cached view of (A, op) and its scratch exist."""
    o = _op(op)
    if Y is None and beta != 0:
        raise ValueError("beta != 0 needs Y")
    i = A.info()
    k = int(k)
    ldx = k if ldx is None else int(ldx)
    ldy = k if ldy is None else int(ldy)
    n_out = i["num_cols"] if o == OP_T else i["num_rows"]
    if Y is None:
        Y = DeviceArray(n_out * max(ldy, 0), OUT_DTYPE[i["dtype"]])
    check(lib().bmsp_spmm_op(A.h, o, float(alpha), X.ptr, ldx, float(beta), Y.ptr, ldy, k, stream))
    return Y


def spmm_op_launch_info(A, op, k, ldx=None, ldy=None):
    """{"kernel", "lanes", "col_chunks", "items", "split_blocks", "view_bytes", "scratch_bytes", "compulsory_bytes"} of the launch
    spmm_op(A, X, k, op) makes; builds the cached view of (A, op) if it is missing (bmsp_spmm_op_launch_info)."""
    o = _op(op)
    info = SpmmOpInfo()
    check(lib().bmsp_spmm_op_launch_info(A.h, o, int(k), int(k if ldx is None else ldx), int(k if ldy is None else ldy), C.byref(info)))
    return info.as_dict()


def _sddmm_args(S, X, Y, k, ldx, ldy, mul_s):
    i = S.info()
    k = int(k)
    ldx = k if ldx is None else int(ldx)
    ldy = k if ldy is None else int(ldy)
    if k < 1 or ldx < k or ldy < k:
        raise ValueError("k must be >= 1 and ldx, ldy >= k (got k = %d, ldx = %d, ldy = %d)" % (k, ldx, ldy))
    dt = np.dtype(NP_DTYPE[i["dtype"]])
    for name, v, rows, ld in (("X", X, i["num_rows"], ldx), ("Y", Y, i["num_cols"], ldy)):
        need = (rows - 1) * ld + k if rows else 0  # (the last row needs no padding)
        if v is None or v.dtype != dt or v.n < need:
            raise ValueError("%s must hold %d rows of %d entries of %s at leading dimension %d" % (name, rows, k, dt.name, ld))
    return i, k, ldx, ldy, SDDMM_MUL_S if mul_s else 0


def sddmm(S, X, Y, k, alpha=1.0, beta=0.0, mul_s=False, transposed=None, ldx=None, ldy=None, stream=None):
    """The sampled dense-dense product on S's pattern as a new matrix (bmsp_sddmm): for every stored (i, j),
    alpha * dot(X[i, :k], Y[j, :k]) + beta * s_ij, or alpha * dot * s_ij with mul_s (beta must then be 0).  X / Y: DeviceArrays of S's
    dtype holding num_rows / num_cols rows, row-major at leading dimension ldx / ldy (default k).  The output has S's structure in layout
    `transposed` (None: S's layout).  Asynchronous on `stream`."""
    i, k, ldx, ldy, flags = _sddmm_args(S, X, Y, k, ldx, ldy, mul_s)
    lay = i["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    check(lib().bmsp_sddmm(S.h, X.ptr, ldx, Y.ptr, ldy, k, float(alpha), float(beta), flags, lay, stream, C.byref(h)))
    return BmSpMatrix(h.value)


def sddmm_values(out, S, X, Y, k, alpha=1.0, beta=0.0, mul_s=False, ldx=None, ldy=None, stream=None):
    """the values of sddmm(S, X, Y, k, ...) into `out`: S itself (in place) or a matrix made from S by sddmm() / scale() / with_layout()
    (bmsp_sddmm_values)."""
    _, k, ldx, ldy, flags = _sddmm_args(S, X, Y, k, ldx, ldy, mul_s)
    check(lib().bmsp_sddmm_values(S.h, X.ptr, ldx, Y.ptr, ldy, k, float(alpha), float(beta), flags, out.h, stream))
    return out


def sddmm_launch_info(S, k, ldx=None, ldy=None, transposed=None):
    """{"kernel", "lanes", "compulsory_bytes"} of the launch sddmm(S, X, Y, k, ldx=ldx, ldy=ldy) makes with 16-byte aligned X and Y
    (bmsp_sddmm_launch_info)."""
    k = int(k)
    lay = S.info()["transposed"] if transposed is None else int(bool(transposed))
    info = SddmmInfo()
    check(lib().bmsp_sddmm_launch_info(S.h, k, k if ldx is None else int(ldx), k if ldy is None else int(ldy), lay, C.byref(info)))
    return info.as_dict()


def _spgemm_masked_args(A, B, M, beta, mul_m, out=None):
    ia, ib, im = A.info(), B.info(), M.info()
    if mul_m and beta != 0:
        raise ValueError("beta must be 0 with mul_m (got %r)" % (beta,))
    if ia["num_cols"] != ib["num_rows"]:
        raise ValueError("A.num_cols (%d) != B.num_rows (%d)" % (ia["num_cols"], ib["num_rows"]))
    if (im["num_rows"], im["num_cols"]) != (ia["num_rows"], ib["num_cols"]):
        raise ValueError("M is %d x %d, A * B is %d x %d" % (im["num_rows"], im["num_cols"], ia["num_rows"], ib["num_cols"]))
    if ia["dtype"] != ib["dtype"]:
        raise ValueError("A and B differ in dtype (%d, %d)" % (ia["dtype"], ib["dtype"]))
    if im["dtype"] != ia["dtype"] and not (ia["dtype"] == F16 and im["dtype"] == F32):
        raise ValueError("M's dtype (%d) must be A's (%d), or F32 for F16 operands" % (im["dtype"], ia["dtype"]))
    if out is not None and (out is A or out is B or (out.h is not None and out.h in (A.h, B.h))):
        raise ValueError("out must not be A or B: the pass would read what it writes")
    return im, MASKED_MUL_M if mul_m else 0


def spgemm_masked(A, B, M, alpha=1.0, beta=0.0, mul_m=False, transposed=None, stream=None):
    """The masked sparse product on M's pattern as a new matrix (bmsp_spgemm_masked): for every stored (i, j) of M,
    alpha * sum_k a_ik * b_kj + beta * m_ij, or alpha * sum * m_ij with mul_m (beta must then be 0); the sum runs over the inner indices
    both operands store, k ascending, one fused multiply-add per product.  A (m x n), B (n x p) and M (m x p) may have either tile layout
    and may be the same matrix; M has A's dtype, or F32 for F16 operands.  The output has M's structure and dtype in layout `transposed`
    (None: M's layout).  Asynchronous on `stream` once B's op-T view exists."""
    im, flags = _spgemm_masked_args(A, B, M, beta, mul_m)
    lay = im["transposed"] if transposed is None else int(bool(transposed))
    h = C.c_void_p()
    check(lib().bmsp_spgemm_masked(A.h, B.h, M.h, float(alpha), float(beta), flags, lay, stream, C.byref(h)))
    return BmSpMatrix(h.value)


def spgemm_masked_values(out, A, B, M, alpha=1.0, beta=0.0, mul_m=False, stream=None):
    """the values of spgemm_masked(A, B, M, ...) into `out`: M itself (in place) or a matrix made from M by spgemm_masked() / sddmm() /
    scale() / with_layout(); never A or B (bmsp_spgemm_masked_values)."""
    _, flags = _spgemm_masked_args(A, B, M, beta, mul_m, out)
    check(lib().bmsp_spgemm_masked_values(A.h, B.h, M.h, float(alpha), float(beta), flags, out.h, stream))
    return out


def spgemm_masked_launch_info(A, B, M, transposed=None):
    """{"kernel", "lanes", "pairs", "view_bytes"} of the launch spgemm_masked(A, B, M) makes; builds B's op-T view if it is missing
    (bmsp_spgemm_masked_launch_info)."""
    im, _ = _spgemm_masked_args(A, B, M, 0.0, False)
    lay = im["transposed"] if transposed is None else int(bool(transposed))
    info = SpgemmMaskedInfo()
    check(lib().bmsp_spgemm_masked_launch_info(A.h, B.h, M.h, lay, C.byref(info)))
    return info.as_dict()


# bmSparse_mult(A, B, C, mode, VERBOSE, tc_version)
def spgemm(A, B, mode=SORT_AUTO, tc_version=5, verbose=False, stream=None):
    h = C.c_void_p()
    st = SpgemmStats()
    check(lib().bmsp_spgemm(A.h, B.h, C.byref(h), int(mode), int(tc_version), int(bool(verbose)), stream, C.byref(st)))
    return BmSpMatrix(h.value), st.as_dict()


def spgemm_symbolic(A, B, mode=SORT_AUTO, tc_version=5, stream=None):
    """C's structure only (values allocated, zero): bmsp_spgemm_symbolic"""
    h = C.c_void_p()
    st = SpgemmStats()
    check(lib().bmsp_spgemm_symbolic(A.h, B.h, C.byref(h), int(mode), int(tc_version), stream, C.byref(st)))
    return BmSpMatrix(h.value), st.as_dict()


def spgemm_numeric(A, B, Cm, tc_version=5, stream=None):
    """the values of A x B into a C that already holds the product's structure: bmsp_spgemm_numeric"""
    st = SpgemmStats()
    check(lib().bmsp_spgemm_numeric(A.h, B.h, Cm.h, int(tc_version), stream, C.byref(st)))
    return st.as_dict()


# bb_segsort(keys, vals, n, segs, length)
def segsort(keys, vals, segs, stream=None):
    """keys: DeviceArray uint64; vals: DeviceArray of 4/8/16-byte items or None; segs: DeviceArray int32."""
    vb = 0 if vals is None else vals.dtype.itemsize
    check(lib().bmsp_segsort_u64(keys.ptr, None if vals is None else vals.ptr, vb, keys.n, segs.ptr, segs.n, stream))


def partition_rows(A, B, parts):
    bounds = np.zeros(parts + 1, dtype=np.int64)
    check(lib().bmsp_partition_rows(A.h, B.h, int(parts), bounds.ctypes.data))
    return bounds


def concat_panels(num_rows, num_cols, panels, dtype=F32):
    """panels: list of (keys, bmps, offsets, values) DeviceArrays (offsets with block_num+1 entries)."""
    P = len(panels)
    bn = np.array([p[0].n for p in panels], dtype=np.int64)
    nz = np.array([p[3].n for p in panels], dtype=np.int64)
    arr = lambda j: (C.c_void_p * P)(*[p[j].ptr for p in panels])
    k, b, o, v = arr(0), arr(1), arr(2), arr(3)
    h = C.c_void_p()
    check(lib().bmsp_matrix_concat_panels(int(num_rows), int(num_cols), P, bn.ctypes.data, nz.ctypes.data, k, b, o, v, dtype,
                                          C.byref(h)))
    return BmSpMatrix(h.value)


class Comm:
    """one RCCL communicator behind the C ABI (bmsp_comm_t): rank 0 makes the id, every rank calls Comm(id, world, rank)."""

    def __init__(self, id_bytes, world, rank):
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(id_bytes), 128)
        check(lib().bmsp_comm_init(buf, int(world), int(rank), C.byref(h)))
        self.h, self.world, self.rank = h.value, int(world), int(rank)

    @classmethod
    def loopback(cls, world):
        """`world` panels computed one after another on the current device, panels moved by device copies (no RCCL)."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().bmsp_comm_init_loopback(int(world), C.byref(h)))
        self.h, self.world, self.rank = h.value, int(world), 0
        return self

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().bmsp_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def from_torch(dist, torch):
        """rendezvous over an existing torch.distributed group (the id travels as 128 bytes in a broadcast)."""
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [Comm.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return Comm(box[0], world, rank)

    def free(self):
        if self.h:
            lib().bmsp_comm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def spgemm_sharded(comm, A, B, mode=SORT_AUTO, tc_version=5, verbose=False, stream=None, gather=True, rounds=0):
    """gather=False: owner keeps (no exchange, the rank's panel of C); rounds: panels per rank whose exchange overlaps the next product (0: library's choice)"""
    h = C.c_void_p()
    st, sh = SpgemmStats(), ShardStats()
    check(lib().bmsp_spgemm_sharded_ex(comm.h, A.h, B.h, C.byref(h), int(mode), int(tc_version), int(bool(verbose)), stream, C.byref(st), C.byref(sh),
                                       int(bool(gather)), int(rounds)))
    return BmSpMatrix(h.value), st.as_dict(), sh.as_dict()


def spmv_sharded(comm, A, v, u=None, variant=0, stream=None):
    i = A.info()
    if u is None:
        u = DeviceArray(i["num_rows"], OUT_DTYPE[i["dtype"]])
    sh = ShardStats()
    check(lib().bmsp_spmv_sharded(comm.h, A.h, v.ptr, u.ptr, int(variant), stream, C.byref(sh)))
    return u, sh.as_dict()


def shard_layout(block_nums, nnzs):
    """(block_start, value_start), parts+1 entries each: where every panel of a sharded product lands (host arithmetic of comm.hip)."""
    bn = np.ascontiguousarray(block_nums, dtype=np.int64)
    nz = np.ascontiguousarray(nnzs, dtype=np.int64)
    b0, z0 = np.zeros(bn.size + 1, np.int64), np.zeros(bn.size + 1, np.int64)
    check(lib().bmsp_shard_layout(int(bn.size), bn.ctypes.data, nz.ctypes.data, b0.ctypes.data, z0.ctypes.data))
    return b0, z0


def shard_row_slices(num_rows, bounds):
    """(row_start, row_count) per panel of a sharded SpMV with block-row bounds `bounds` (parts+1 entries)."""
    b = np.ascontiguousarray(bounds, dtype=np.int64)
    rs, rc = np.zeros(b.size - 1, np.int64), np.zeros(b.size - 1, np.int64)
    check(lib().bmsp_shard_row_slices(int(num_rows), int(b.size - 1), b.ctypes.data, rs.ctypes.data, rc.ctypes.data))
    return rs, rc


class CSRMatrix:
    """mirror of the reference's CSRMatrix (include/CSRMatrix.h:13-21)."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def from_mtx(path):
        h = C.c_void_p()
        check(lib().bmsp_csr_from_mtx(os.fsencode(path), C.byref(h)))
        return CSRMatrix(h.value)

    @staticmethod
    def from_arrays(num_rows, num_cols, row_offsets, cols, vals):
        ro = np.ascontiguousarray(row_offsets, dtype=np.int32)
        c = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=np.float32)
        h = C.c_void_p()
        check(lib().bmsp_csr_from_arrays(int(num_rows), int(num_cols), c.size, ro.ctypes.data, c.ctypes.data, v.ctypes.data, C.byref(h)))
        return CSRMatrix(h.value)

    def arrays(self):
        nr, nc, nnz = C.c_int(), C.c_int(), C.c_int64()
        check(lib().bmsp_csr_info(self.h, C.byref(nr), C.byref(nc), C.byref(nnz)))
        ro, c, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().bmsp_csr_arrays(self.h, C.byref(ro), C.byref(c), C.byref(v)))
        n = nnz.value
        f = lambda p, cnt, ct, dt: (np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (cnt,)).copy() if cnt else np.zeros(0, dt))
        return nr.value, nc.value, f(ro, nr.value + 1, C.c_int, np.int32), f(c, n, C.c_int, np.int32), f(v, n, C.c_float, np.float32)

    def multiply(self, other):
        h = C.c_void_p()
        check(lib().bmsp_csr_multiply(self.h, other.h, C.byref(h)))
        return CSRMatrix(h.value)

    def multiply_host(self, other, threads=0):
        """cusp::multiply's host path (no GPU call)."""
        h = C.c_void_p()
        check(lib().bmsp_csr_multiply_host(self.h, other.h, C.byref(h), int(threads)))
        return CSRMatrix(h.value)

    def shape(self):
        nr, nc, nnz = C.c_int(), C.c_int(), C.c_int64()
        check(lib().bmsp_csr_info(self.h, C.byref(nr), C.byref(nc), C.byref(nnz)))
        return nr.value, nc.value, nnz.value

    def spmv_host(self, x, threads=0):
        nr = self.shape()[0]
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty(nr, dtype=np.float32)
        check(lib().bmsp_csr_spmv_host(self.h, x.ctypes.data, y.ctypes.data, int(threads)))
        return y

    def spmv(self, x):
        nr = self.shape()[0]
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty(nr, dtype=np.float32)
        check(lib().bmsp_csr_spmv(self.h, x.ctypes.data, y.ctypes.data))
        return y

    def __del__(self):
        try:
            if self.h:
                lib().bmsp_csr_free(self.h)
                self.h = None
        except Exception:
            pass
