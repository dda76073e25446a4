"""uspmv_dist_check_arrays: the bitwise self-check of a distributed object against the block in HBM.  Loopback objects,
P = 3, seg-rows on the (16,16,24) stencil with decades 0, each built by from_device_arrays from the block uspmv_gen_stencil27_device made:
clean, the checksum bit for bit that of uspmv_dist_check with the host block, and not vacuous -- one flipped sign is one mismatching row."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GRID, P, C, SIGMA = (16, 16, 24), 3, 32, 512
N = GRID[0] * GRID[1] * GRID[2]
UNSUPPORTED = 3


def _pkg():
    import __graft_entry__ as ge
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def setting():
    """(wsa, the 0.7 quantile of |v| over the whole matrix)"""
    pkg = _pkg()
    m = pkg.gen_stencil27(*GRID)
    wsa = pkg.seg_work_sharing_arr(m, "seg-rows", P)
    assert np.array_equal(np.diff(wsa), np.full(P, N // P))
    return wsa, float(np.quantile(np.abs(np.asarray(m.arrays()[2])), 0.7))


def kind_kw(pkg, kind):
    return {"dp": dict(dtype=pkg.F64), "sp": dict(dtype=pkg.F32), "dp_sp": dict(ap_threshold=setting()[1])}[kind]


def make(pkg, rank, **kw):
    """the object from the device-generated block: (object, device arrays, the host block)"""
    wsa, _ = setting()
    rb, re_ = int(wsa[rank]), int(wsa[rank + 1])
    dev = pkg.gen_stencil27_device(*GRID, row_begin=rb, row_end=re_)
    d = pkg.DistNative.from_device_arrays(*dev, N, wsa, C, SIGMA, rank, P, None, comm_rank=0, comm_size=1, exchange="peer", **kw)
    assert d.loopback and d.n_halo > 0
    return d, dev, pkg.gen_stencil27(*GRID, row_begin=rb, row_end=re_)


@pytest.mark.parametrize("kind", ("dp", "sp", "dp_sp"))
def test_check_arrays_is_clean_and_gives_the_host_checks_checksum(pkg, kind):
    import torch as t
    t.cuda.set_device(0)
    for rank in range(P):
        d, dev, loc = make(pkg, rank, **kind_kw(pkg, kind))
        x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
        bad_h, cs_h = d.check(loc, x, y)
        bad_d, cs_d = d.check_arrays(*dev, x, y)
        assert bad_h == 0 and bad_d == 0, (kind, rank, bad_h, bad_d)
        assert np.float64(cs_d).view(np.uint64) == np.float64(cs_h).view(np.uint64), (kind, rank, cs_d, cs_h)
        assert cs_d != 0.0
        d.close()


@pytest.mark.parametrize("kind", ("dp", "sp", "dp_sp"))
def test_one_flipped_sign_is_one_mismatching_row(pkg, kind):
    """rank 1 (halo on both sides): an entry of a chosen row whose column is local, then one whose column lies in the halo"""
    import torch as t
    t.cuda.set_device(0)
    rank = 1
    wsa, _ = setting()
    d, (dI, dJ, dV), _ = make(pkg, rank, **kind_kw(pkg, kind))
    I, J = dI.cpu().numpy(), dJ.cpu().numpy()
    local_col = (J >= wsa[rank]) & (J < wsa[rank + 1])
    row = 777
    picks = (int(np.flatnonzero((I == row) & local_col)[3]), int(np.flatnonzero(~local_col)[5]))
    assert not local_col[picks[1]] and local_col[picks[0]]
    x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
    for k in picks:
        V2 = dV.clone()
        V2[k] = -V2[k]
        assert float(V2[k]) != 0.0
        bad, _ = d.check_arrays(dI, dJ, V2, x, y)
        assert bad == 1, (kind, k, bad)
    assert d.check_arrays(dI, dJ, dV, x, y)[0] == 0
    d.close()


def test_check_arrays_refuses_an_object_with_an_fp16_part(pkg):
    import torch as t
    t.cuda.set_device(0)
    d, dev, _ = make(pkg, 0, ap_kind="dp_hp", ap_threshold=setting()[1])
    x, y = d.new_x(np.zeros(d.n_local)), d.new_y()
    with pytest.raises(pkg.UspmvError, match=r"ap\[dp_hp\]") as e:
        d.check_arrays(*dev, x, y)
    assert e.value.status == UNSUPPORTED
    d.close()
