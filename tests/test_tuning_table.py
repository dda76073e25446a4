"""uspmv_set_tuning / uspmv_get_tuning against a table recorded from the library before the keys moved into one static table
(tests/golden/tuning_table.json, whose header names the commit): for every key and probe value the status of set, the value get
returns afterwards and the text of a refusal must be what they were.  Host-only code: runs without a GPU."""
import ctypes as C
import json
import os

from conftest import GOLDEN

PROBES = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 32, 63, 64, 65, 99, 100, 128, 256, 512, 1024, 2047, 2048, 4096, 16384, 65536,
          65537, 1 << 20]


def _table():
    with open(os.path.join(GOLDEN, "tuning_table.json")) as f:
        return json.load(f)


def _get(L, key):
    v = C.c_int(0)
    assert L.uspmv_get_tuning(key.encode(), C.byref(v)) == 0, key
    return v.value


def test_fixture_covers_the_probes():
    t = _table()
    assert t["probes"] == PROBES
    assert len(t["keys"]) == 52
    assert all(len(k["rows"]) == len(PROBES) for k in t["keys"].values())


def test_every_key_sets_and_gets_as_recorded(pkg):
    L = pkg.lib()
    t = _table()
    wrong = []
    for key, rec in t["keys"].items():
        default = _get(L, key)
        try:
            if default != rec["default"]:
                wrong.append((key, "default", default, rec["default"]))
            for v, (status, after) in zip(t["probes"], rec["rows"]):
                assert L.uspmv_set_tuning(key.encode(), default) == 0 and _get(L, key) == default, key   # each probe starts from the default
                rc = L.uspmv_set_tuning(key.encode(), v)
                got = [rc, _get(L, key)]
                if got != [status, after]:
                    wrong.append((key, v, got, [status, after]))
                if rc and L.uspmv_last_error().decode() != rec["error"]:
                    wrong.append((key, v, L.uspmv_last_error().decode(), rec["error"]))
        finally:
            assert L.uspmv_set_tuning(key.encode(), default) == 0 and _get(L, key) == default, key
    assert not wrong, wrong


def test_unknown_key_fails_in_set_and_get(pkg):
    L = pkg.lib()
    v = C.c_int(-7)
    assert L.uspmv_set_tuning(b"no_such_key", 1) != 0
    assert L.uspmv_last_error().decode() == "uspmv_set_tuning: unknown key 'no_such_key'"
    assert L.uspmv_get_tuning(b"no_such_key", C.byref(v)) != 0
    assert L.uspmv_last_error().decode() == "uspmv_get_tuning: unknown key 'no_such_key'"
    assert v.value == -7
    assert L.uspmv_set_tuning(None, 1) != 0 and L.uspmv_get_tuning(None, C.byref(v)) != 0 and L.uspmv_get_tuning(b"unroll", None) != 0
