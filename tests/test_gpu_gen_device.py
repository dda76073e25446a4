"""uspmv_gen_stencil27_device (csrc/gen_kernels.hip) against uspmv_gen_stencil27: I, J and V equal in every bit (V on
its bit pattern), on grids where every row is a boundary case, on one with several workgroups in every kernel, for dof 1 and 3, two seeds
and row ranges that begin and end inside a node."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GRIDS = ((1, 1, 1), (2, 1, 1), (1, 3, 1), (3, 3, 3), (5, 4, 3), (16, 16, 24))
SEEDS = (0x5EED, 0x0123456789ABCDEF)


def _pkg():
    import __graft_entry__ as ge
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def host_matrix(grid, dof, seed):
    """the whole matrix from the host generator, once per (grid, dof, seed): (row starts, I, J, V)"""
    m = _pkg().gen_stencil27(*grid, dof=dof, seed=seed)
    I, J, V = (np.array(a) for a in m.arrays())
    start = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=m.n_rows))))
    return start, I, J, V


def ranges(pkg, grid, dof):
    nx, ny, nz = grid
    n = nx * ny * nz * dof
    out = {(0, n)}
    if dof == 3 and n - 2 > 4:
        out.add((4, n - 2))                                  # begins and ends inside a node
    node = lambda x, y, z: x + nx * (y + ny * z)
    corner, edge, inner = node(0, 0, 0), node(min(1, nx - 1), 0, 0), node(min(1, nx - 1), min(1, ny - 1), min(1, nz - 1))
    for nd, d in ((corner, 0), (edge, dof - 1), (inner, dof // 2), (nx * ny * nz - 1, dof - 1)):
        out.add((nd * dof + d, nd * dof + d + 1))            # one single row
    if grid == (16, 16, 24):
        w = pkg.seg_from_row_counts(pkg.gen_stencil27_row_counts(nx, ny, nz, dof), "seg-nnz", 3)
        assert len(set(np.diff(w))) > 1                      # unequal blocks
        out.update((int(w[p]), int(w[p + 1])) for p in range(3))
    return sorted(out)


@pytest.mark.parametrize("dof", (1, 3))
@pytest.mark.parametrize("grid", GRIDS)
def test_device_generator_equals_the_host_generator_bit_for_bit(pkg, grid, dof):
    import torch as t
    t.cuda.set_device(0)
    n_cases = 0
    for seed in SEEDS:
        start, I, J, V = host_matrix(grid, dof, seed)
        for rb, re_ in ranges(pkg, grid, dof):
            dI, dJ, dV = pkg.gen_stencil27_device(*grid, dof=dof, seed=seed, row_begin=rb, row_end=re_)
            k0, k1 = int(start[rb]), int(start[re_])
            tag = (grid, dof, hex(seed), rb, re_)
            assert dI.numel() == dJ.numel() == dV.numel() == k1 - k0, tag      # the dcoo's nnz equals the host's
            assert np.array_equal(dI.cpu().numpy(), I[k0:k1] - rb), tag
            assert np.array_equal(dJ.cpu().numpy(), J[k0:k1]), tag
            assert np.array_equal(dV.cpu().numpy().view(np.int64), V[k0:k1].view(np.int64)), tag
            n_cases += 1
    assert n_cases >= len(SEEDS)


def test_a_block_equals_the_host_call_on_that_block(pkg):
    """... and against uspmv_gen_stencil27(row_begin, row_end) itself, not a slice of the whole matrix: (16,16,24), dof 3, a block that
    begins and ends inside a node; about 150 k entries, several workgroups in every kernel"""
    import torch as t
    t.cuda.set_device(0)
    grid, dof = (16, 16, 24), 3
    n = 16 * 16 * 24 * dof
    rb, re_ = n // 3 + 1, 2 * n // 3 + 2
    m = pkg.gen_stencil27(*grid, dof=dof, row_begin=rb, row_end=re_)
    I, J, V = m.arrays()
    dI, dJ, dV = pkg.gen_stencil27_device(*grid, dof=dof, row_begin=rb, row_end=re_)
    assert m.nnz == dI.numel() > 150000
    assert np.array_equal(dI.cpu().numpy(), I) and np.array_equal(dJ.cpu().numpy(), J)
    assert np.array_equal(dV.cpu().numpy().view(np.int64), np.asarray(V).view(np.int64))


def test_decades_are_refused_on_the_device_too(pkg):
    with pytest.raises(pkg.UspmvError, match="magnitude_decades") as e:
        pkg.gen_stencil27_device(4, 4, 4, magnitude_decades=4.0)
    assert e.value.status == 3
