"""The refusals the three set-ups of a distributed object from a COO block (uspmv_dist_create_from_coo, _ap_from_coo, _ap_hp_from_coo and
their _ex forms) share, and the one each has of its own: exact texts under the function's own name.  All of them come before the first
collective and before the device is asked for, so this runs without a GPU."""
import ctypes

import numpy as np
import pytest

ONE, AP, AP_HP = "uspmv_dist_create_from_coo", "uspmv_dist_create_ap_from_coo", "uspmv_dist_create_ap_hp_from_coo"
LAST_BLOCK = " (the reference's seg methods only repair an empty LAST block, code/mpi_funcs.hpp:602-606)"
AP_DP_HP, AP_DP_SP = 0, 3                   # USPMV_AP_* of include/uspmv.h


@pytest.fixture(scope="module")
def block(pkg):
    coo = pkg.gen_stencil27(1, 2, 3)
    assert coo.n_rows == 6
    return coo, np.array([0, 6], np.int32)


def _create(pkg, who, ex, rank, P, local, wsa, out, dtype=None, kind=AP_DP_HP):
    """the status and message of creator `who` (its _ex form when ex) on (local, wsa); C 2, sigma 2, thresholds 1.0 / 0.1, tile plan on"""
    from ultimate_spmv_amd import binding as B
    assert (pkg.AP_DP_HP, pkg.AP_DP_SP) == (AP_DP_HP, AP_DP_SP)
    head = (None, rank, P, rank, P, None if local is None else local.h, None if wsa is None else B._np_ptr(wsa), 2, 2)
    own = {ONE: (pkg.F64 if dtype is None else dtype,), AP: (1.0,), AP_HP: (kind, 1.0, 0.1)}[who]
    h = ctypes.c_void_p()
    tail = ((None,) if ex else ()) + (ctypes.byref(h) if out else None,)
    rc = getattr(B.lib(), who + ("_ex" if ex else ""))(*head, *own, 1, *tail)
    assert rc != 0 and not h.value
    return rc, B.lib().uspmv_last_error().decode()


@pytest.mark.parametrize("ex", [True, False], ids=["ex", "plain"])
@pytest.mark.parametrize("who", [ONE, AP, AP_HP])
def test_the_shared_refusals_carry_the_creators_name(pkg, block, who, ex):
    coo, wsa = block
    for local, w, out in ((None, wsa, True), (coo, None, True), (coo, wsa, False)):
        assert _create(pkg, who, ex, 0, 1, local, w, out) == (1, f"{who}: NULL argument")
    wsa3 = np.array([0, 3, 3, 6], np.int32)
    for rank, P in ((3, 3), (5, 3), (-1, 3), (0, 0)):
        assert _create(pkg, who, ex, rank, P, coo, wsa3, True) == (1, f"{who}: bad rank / P")
    for rank in range(3):                                   # every rank refuses the empty MIDDLE block alike
        want = f"{who}: block 1 of 3 owns no rows (work_sharing_arr 3 .. 3) -- fewer ranks or another partition" + (LAST_BLOCK if who == ONE else "")
        assert _create(pkg, who, ex, rank, 3, coo, wsa3, True) == (1, want)


@pytest.mark.parametrize("ex", [True, False], ids=["ex", "plain"])
def test_each_creators_own_refusal(pkg, block, ex):
    coo, wsa = block
    assert _create(pkg, ONE, ex, 0, 1, coo, wsa, True, dtype=7) == (1, f"{ONE}: unknown dtype 7")
    assert _create(pkg, AP_HP, ex, 0, 1, coo, wsa, True, kind=41) == (1, f"{AP_HP}: unknown kind 41")
    assert _create(pkg, AP_HP, ex, 0, 1, coo, wsa, True, kind=AP_DP_SP) == (
        1, f"{AP_HP}: ap[dp_sp] has no fp16 part; its object is made by uspmv_dist_create_ap_from_coo")
    # ... each after the NULL and rank checks, before the empty-block one
    assert _create(pkg, ONE, ex, 0, 1, None, wsa, True, dtype=7)[1] == f"{ONE}: NULL argument"
    assert _create(pkg, AP_HP, ex, 2, 2, coo, wsa, True, kind=41)[1] == f"{AP_HP}: bad rank / P"
    wsa3 = np.array([0, 3, 3, 6], np.int32)
    assert _create(pkg, ONE, ex, 0, 3, coo, wsa3, True, dtype=7)[1] == f"{ONE}: unknown dtype 7"
    assert _create(pkg, AP_HP, ex, 0, 3, coo, wsa3, True, kind=41)[1] == f"{AP_HP}: unknown kind 41"
