"""What the set-up of a distributed object from a COO block leaves behind, for the five kinds of object (one precision, ap[dp_sp], ap[dp_hp],
ap[sp_hp], ap[dp_sp_hp]) with and without the tile plan: whether the step runs on tile lists, the interior / boundary / padding-only /
real-boundary counts, the halo and the vector length -- against literals -- and the bitwise self-check in the default and the plain form.
Loopback on one GPU, seg-rows, the smallest blocks of test_gpu_dist_ap_hp.py (27 and 6.3 tiles of 256 rows)."""
import pytest

from test_dist_ap_hp_host import DEC, T1, T2

pytestmark = pytest.mark.gpu

KINDS = ("dp", "dp_sp", "dp_hp", "sp_hp", "dp_sp_hp")
CASES = {2: ((24, 24, 24), 32, 512), 3: ((20, 9, 27), 16, 64)}        # P: (stencil nodes, C, sigma)
FIELDS = ("use_tiles", "n_interior", "n_boundary", "pad_tiles", "real_boundary_tiles", "n_halo", "n_send", "padded_vec_size")

# (kind, tlc, P) -> per rank, the FIELDS.  Recorded on commit f13f8c1 (the three separate creators) by running observe() below over this
# parametrisation; the code under test never writes this table.
EXPECT = {
    ('dp', True, 2): ((True, 24, 3, 0, 3, 576, 576, 7488), (True, 10, 17, 13, 4, 577, 577, 7489),),
    ('dp', True, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 49, 53, 0, 53, 361, 361, 1981), (False, 57, 45, 0, 45, 181, 181, 1801),),
    ('dp', False, 2): ((False, 194, 22, 0, 22, 576, 576, 7488), (False, 169, 47, 0, 47, 577, 577, 7489),),
    ('dp', False, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 49, 53, 0, 53, 361, 361, 1981), (False, 57, 45, 0, 45, 181, 181, 1801),),
    ('dp_sp', True, 2): ((True, 24, 3, 0, 3, 576, 576, 7488), (True, 0, 27, 23, 4, 577, 577, 7489),),
    ('dp_sp', True, 3): ((True, 5, 2, 0, 2, 180, 180, 1800), (True, 0, 7, 4, 3, 361, 361, 1981), (True, 0, 7, 6, 1, 181, 181, 1801),),
    ('dp_sp', False, 2): ((False, 192, 24, 0, 24, 576, 576, 7488), (False, 4, 212, 0, 212, 577, 577, 7489),),
    ('dp_sp', False, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 0, 102, 0, 102, 361, 361, 1981), (False, 0, 102, 0, 102, 181, 181, 1801),),
    ('dp_hp', True, 2): ((True, 24, 3, 0, 3, 576, 576, 7488), (True, 0, 27, 23, 4, 577, 577, 7489),),
    ('dp_hp', True, 3): ((True, 5, 2, 0, 2, 180, 180, 1800), (True, 0, 7, 4, 3, 361, 361, 1981), (True, 0, 7, 6, 1, 181, 181, 1801),),
    ('dp_hp', False, 2): ((False, 192, 24, 0, 24, 576, 576, 7488), (False, 4, 212, 0, 212, 577, 577, 7489),),
    ('dp_hp', False, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 0, 102, 0, 102, 361, 361, 1981), (False, 0, 102, 0, 102, 181, 181, 1801),),
    ('sp_hp', True, 2): ((True, 24, 3, 0, 3, 576, 576, 7488), (True, 0, 27, 23, 4, 577, 577, 7489),),
    ('sp_hp', True, 3): ((True, 5, 2, 0, 2, 180, 180, 1800), (True, 0, 7, 4, 3, 361, 361, 1981), (True, 0, 7, 6, 1, 181, 181, 1801),),
    ('sp_hp', False, 2): ((False, 192, 24, 0, 24, 576, 576, 7488), (False, 4, 212, 0, 212, 577, 577, 7489),),
    ('sp_hp', False, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 0, 102, 0, 102, 361, 361, 1981), (False, 0, 102, 0, 102, 181, 181, 1801),),
    ('dp_sp_hp', True, 2): ((True, 24, 3, 0, 3, 576, 576, 7488), (True, 0, 27, 23, 4, 577, 577, 7489),),
    ('dp_sp_hp', True, 3): ((True, 5, 2, 0, 2, 180, 180, 1800), (True, 0, 7, 4, 3, 361, 361, 1981), (True, 0, 7, 6, 1, 181, 181, 1801),),
    ('dp_sp_hp', False, 2): ((False, 192, 24, 0, 24, 576, 576, 7488), (False, 0, 216, 0, 216, 577, 577, 7489),),
    ('dp_sp_hp', False, 3): ((False, 88, 14, 0, 14, 180, 180, 1800), (False, 0, 102, 0, 102, 361, 361, 1981), (False, 0, 102, 0, 102, 181, 181, 1801),),
}
# What the table shows: the one-precision block of 24 x 24 x 12 nodes holds all three tile classes on rank 1 (10 interior, 13 padding-only,
# 4 real boundary); its 1 620-row block at C 16 stages no tile and runs on chunk lists even with the plan asked for.  A split has no
# interior tile on a rank >= 1 of these blocks: every 256-row tile holds a chunk that is padded in one of the parts.


def make(pkg, kind, tlc, P, rank):
    shape, C, sigma = CASES[P]
    wsa = pkg.seg_from_row_counts(pkg.gen_stencil27_row_counts(*shape), "seg-rows", P)
    loc = pkg.gen_stencil27(*shape, magnitude_decades=DEC, row_begin=int(wsa[rank]), row_end=int(wsa[rank + 1]))
    ap = {"dp": {}, "dp_sp": dict(ap_threshold=T1)}.get(kind, dict(ap_kind=kind, ap_threshold=T1, ap_threshold_2=T2))
    return loc, pkg.DistNative(loc, wsa, C, sigma, rank, P, pkg.comm_unique_id(), comm_rank=0, comm_size=1, tlc=tlc, **ap)


def observe(d):
    info = d.pad_info()
    return (d.use_tiles, d.n_interior, d.n_boundary, info["pad_tiles"], info["real_boundary_tiles"], d.n_halo, d.n_send, d.padded_vec_size)


def test_the_table_covers_the_parametrisation_and_every_tile_class():
    assert set(EXPECT) == {(k, t, P) for k in KINDS for t in (True, False) for P in CASES}
    seen = set()
    for (kind, tlc, P), ranks in EXPECT.items():
        assert len(ranks) == P
        for rank, row in enumerate(ranks):
            use_tiles, n_int, n_bnd, n_pad, n_real = row[:5]
            assert (not use_tiles or tlc) and n_real == n_bnd - n_pad and (use_tiles or n_pad == 0), (kind, tlc, P, rank)
            if use_tiles and rank >= 1:
                seen |= {name for name, n in (("interior", n_int), ("padding-only", n_pad), ("real boundary", n_real)) if n > 0}
    assert seen == {"interior", "padding-only", "real boundary"}


@pytest.mark.parametrize("P", sorted(CASES))
@pytest.mark.parametrize("tlc", [True, False], ids=["tlc", "chunks"])
@pytest.mark.parametrize("kind", KINDS)
def test_set_up_leaves_the_recorded_lists_and_a_step_that_checks(pkg, kind, tlc, P):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    for rank in range(P):
        loc, d = make(pkg, kind, tlc, P, rank)
        got = observe(d)
        assert got == EXPECT[(kind, tlc, P)][rank], (kind, tlc, P, rank, dict(zip(FIELDS, got)))
        nl = d.n_local
        assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] == 0                  # the object's default form
        d.set_option("overlap", 0)
        assert d.check(loc, d.new_x(np.zeros(nl)), d.new_y())[0] == 0                  # plain: exchange, then the whole matrix
        d.close()
