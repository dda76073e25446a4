"""The peer-store exchange's interface without a GPU: the C enum, the getter the library exports, and the Python argument checks that
run before anything touches a device."""
import os
import re

import pytest

from conftest import ROOT


def test_the_peer_exchange_is_part_of_the_c_abi(pkg):
    h = open(os.path.join(ROOT, "include", "uspmv.h")).read()
    assert re.search(r"USPMV_EXCHANGE_RCCL = 0, USPMV_EXCHANGE_HOST = 1, USPMV_EXCHANGE_PEER = 2", h)
    assert "int uspmv_dist_exchange(const uspmv_dist_t *d, int *exchange);" in h
    assert (pkg.EXCHANGE_RCCL, pkg.EXCHANGE_HOST, pkg.EXCHANGE_PEER) == (0, 1, 2)
    from ultimate_spmv_amd import binding as B
    assert B.EXCHANGES == ("rccl", "host", "peer")
    assert pkg.lib().uspmv_dist_exchange(None, None) == 1          # NULL arguments: USPMV_ERR_INVALID, no device needed


def test_dist_native_checks_the_exchange_argument(pkg):
    coo = pkg.gen_stencil27(4, 4, 4)
    wsa = [0, 32, 64]
    with pytest.raises(ValueError, match="one of"):
        pkg.DistNative(coo, wsa, 32, 512, 0, 2, exchange="nccl")
    with pytest.raises(ValueError, match="one of"):
        pkg.DistNative(coo, wsa, 32, 512, 0, 2, host_exchange=True, exchange="peer")
    with pytest.raises(ValueError, match="needs a HostComm"):
        pkg.DistNative(coo, wsa, 32, 512, 0, 2, host_exchange=True)
