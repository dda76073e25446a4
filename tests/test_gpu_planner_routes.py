"""The SpMV planner's routes, pinned per entry: tests/golden/planner_routes.json holds, for every public planner entry (optimize /
optimize_device, optimize_ap / optimize_device_ap, optimize_ap_hp / optimize_device_ap_hp for the three kinds with an fp16 part) on the
smallest matrices that reach each route -- the line plan, the line plan on grown tiles, the plan over single x elements, the column-window
sweep, and the line plan a split with an fp16 part drops (staged on some but under half of its tiles, the sweep declining) -- what the entry
returned, what the handles carry afterwards and a sha1 over the plan's arrays, as tools/planner_routes.py recorded them BEFORE the planner's
entries were folded into one driver (csrc/tlc_planner.hip: plan_parts).  Every record is recomputed here and compared for equality."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("planner_routes", os.path.join(ROOT, "tools", "planner_routes.py"))
routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(routes)

with open(os.path.join(GOLDEN, "planner_routes.json")) as _f:
    TABLE = json.load(_f)
WANT = {r["case"]: r for r in TABLE["records"]}


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return torch


def test_the_table_covers_every_route_of_every_entry():
    """the conditions the table was recorded under (no GPU needed, but the table is this module's)"""
    assert len(WANT) == len(TABLE["records"]) == len(routes.cases(TABLE))
    for kind in routes.KINDS:
        for planner in routes.PLANNERS:
            recs = {route: WANT[f"{route}/{kind}/{planner}"] for route in TABLE["sizes"]}
            assert {i[0] for i in recs["lines"]["plan_info"]} == {1} and set(recs["lines"]["granularity"]) == {16}
            assert {i[0] for i in recs["elements"]["plan_info"]} == {1} and set(recs["elements"]["granularity"]) == {1}
            assert {i[0] for i in recs["sweep"]["plan_info"]} == {2}
            if kind.endswith("_hp"):
                r = recs["dropped"]
                assert {i[0] for i in r["plan_info"]} == {0} and 0 < 2 * r["returned"][1] < r["returned"][0]
        for route in TABLE["sizes"]:
            assert WANT[f"{route}/{kind}/host"]["sha1"] == WANT[f"{route}/{kind}/device"]["sha1"], (route, kind)
    assert any(max(r["tile_rows"]) > 256 for r in WANT.values())


@pytest.mark.parametrize("route,size,kind,planner", [pytest.param(*c, id=f"{c[0]}-{c[2]}-{c[3]}") for c in routes.cases(TABLE)])
def test_route_is_the_recorded_one(pkg, gpu, route, size, kind, planner):
    got = routes.record(pkg, route, size, kind, planner)
    assert got == WANT[got["case"]]
