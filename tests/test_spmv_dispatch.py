"""bmsp_spmv's kernel decision is ONE function (choose() in csrc/spmv.hip), shared by the launcher, bmsp_spmv_launch_info,
bmsp_spmv_chunk_layout and bmsp_matrix_prepare.  What it reports must therefore not depend on what was asked of the handle before:

three handles from the same arrays -- one untouched, one after prepare(1), one after a first bmsp_spmv -- give the same launch-info dict
(kernel, compulsory_bytes, format_bytes) and the same chunk layout, their products are bit-identical, and asking again after the product
gives the same dict once more.  Every launch of util.SPMV_LAUNCHES in every dtype its kernel exists for, and a row-panel view of the
sparse gap matrix under the default variant; one test per dtype, the launches inside it, each under its own environment.

Values are small positive integers (test_streams.mvals / vec): every sum is exact in any order, so bit equality also holds for the
kernels whose LDS float adds have no fixed order."""
import numpy as np
import pytest

import util
from util import SPMV_LAUNCHES, SPMV_CHUNK_LAYOUT
from test_streams import structure, mvals, vec, mat, dev, NPDT, OUTDT, DT

VIEW = "view_default"    # block-rows [lo, hi) of the sparse gap matrix: the position cache of a view starts at the view's first value


def check_launch(bmsp, launch, dtype):
    kind, env, variant, kernel = SPMV_LAUNCHES[launch] if launch != VIEW else ("sparse", {}, 0, "spmv_vstream_kernel<kCached, ")
    S = structure(kind)
    nr, nc = S[:2]
    nbr = (nr + 7) // 8
    lo, hi = (nbr // 3, 2 * nbr // 3) if launch == VIEW else (0, nbr)
    parents = [mat(bmsp, S, 0, dtype) for _ in range(3)]
    untouched, prepared, called = [A.row_panel(lo, hi) for A in parents] if launch == VIEW else parents
    x = dev(bmsp, vec(nc, 0), NPDT[dtype])

    def product(A):
        y = bmsp.DeviceArray(nr, OUTDT[dtype])
        bmsp.check(bmsp.lib().bmsp_memset(y.ptr, 0xFF, nr * y.dtype.itemsize))
        bmsp.check(bmsp.lib().bmsp_spmv(A.h, x.ptr, y.ptr, variant, None))
        return y.to_host()[lo * 8:min(hi * 8, nr)]    # (a view writes its own rows only)

    def report(A):
        return bmsp.spmv_launch_info(A, variant), bmsp.spmv_chunk_layout(A)

    prepared.prepare(1)
    first = product(called)
    reports = [report(A) for A in (untouched, prepared, called)]
    assert reports[0][0]["kernel"].startswith(kernel), (launch, reports[0])
    assert reports[0][1] == SPMV_CHUNK_LAYOUT.get(launch, 0), (launch, reports[0])
    assert reports[1] == reports[0] and reports[2] == reports[0], (launch, reports)
    assert reports[0][0]["compulsory_bytes"] > 0 and reports[0][0]["format_bytes"] > 0, (launch, reports[0])
    ys = [product(A) for A in (untouched, prepared, called)]
    ref = (util.scipy_csr(nr, nc, S[2], S[3], mvals(S, 0)) @ vec(nc, 0))[lo * 8:min(hi * 8, nr)]
    for y in [first] + ys:
        np.testing.assert_array_equal(y.view(np.uint8), ys[0].view(np.uint8), err_msg=launch)
    np.testing.assert_array_equal(ys[0].astype(np.float64), ref, err_msg=launch)
    assert [report(A) for A in (untouched, prepared, called)] == reports, launch


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1, 2], ids=[DT[d] for d in (0, 1, 2)])
def test_report_does_not_depend_on_history(bmsp, monkeypatch, dtype):
    launches = [l for l, d in util.spmv_launch_params((dtype,))] + [VIEW]
    assert len(launches) >= 12
    for launch in launches:
        with monkeypatch.context() as m:
            for k, v in ({} if launch == VIEW else SPMV_LAUNCHES[launch][1]).items():
                m.setenv(k, v)
            check_launch(bmsp, launch, dtype)
