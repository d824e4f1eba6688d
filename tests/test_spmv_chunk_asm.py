"""Resources of the chunked SpMV sweep in the gfx950 assembly (no GPU needed): spmv.hip is compiled device-only with the Makefile's own
compile line, as test_fold_handoff_asm.py does, and every instantiation of spmv_chunk_kernel -- the round-7 body and the row-sorted one --
must keep to 64 VGPRs (8 waves per SIMD), use no scratch, and hold no LDS float add (ds_add_f32 is paid per active lane: DESIGN.md,
rounds 6 and 7)."""
import re

import pytest

from test_fold_handoff_asm import functions, to_asm

KERNEL = "17spmv_chunk_kernel"


@pytest.fixture(scope="module")
def chunk_kernels(tmp_path_factory):
    path = to_asm("spmv", str(tmp_path_factory.mktemp("chunk_asm")))
    text = open(path).read()
    out = {}
    for name, body in functions(path).items():
        if KERNEL in name:
            res = {k: int(re.search(r"^\s*\.set %s\.%s, (\d+)" % (re.escape(name), k), text, re.M).group(1)) for k in ("num_vgpr", "num_agpr", "private_seg_size")}
            out[name] = (body, res)
    return out


def test_both_bodies_are_instantiated(chunk_kernels):
    assert any(KERNEL + "ILb0E" in n for n in chunk_kernels) and any(KERNEL + "ILb1E" in n for n in chunk_kernels), sorted(chunk_kernels)


def test_registers_scratch_and_lds_adds(chunk_kernels):
    for name, (body, res) in chunk_kernels.items():
        assert res["num_vgpr"] + res["num_agpr"] <= 64, (name, res)
        assert res["private_seg_size"] == 0, (name, res)
        assert not [ln for ln in body if re.match(r"\s*scratch_", ln)], name
        assert not [ln for ln in body if re.match(r"\s*ds_add(_rtn)?_f32", ln)], name
