"""tests/stale_lobby_scenarios.py under the CPU shim and on the literal restatement: a stored lobby that a cancel left
stale, the anchor's move in every kernel's stored-lobby fill (k_walk, tc_chaser's inline fill, kt_late's head_fill).
The device's twin is tests/test_gpu_stale_lobby.py."""
import pytest

import stale_lobby_scenarios as S
from emu_engine import EmuEngine, EmuEngineSmall

SMALL = S.SMALL_SIZE
PRODUCT_TUNINGS = [({}, "default"), ({"team_late0": 10000000}, "late0=1e7"), ({"team_late": 0, "team_split": 0}, "late=0")]


def test_every_axis_value_appears():
    assert S.axis_values() == ["A1", "A2", "A3", "A4", "A5", "B1", "B2", "B3", "B4", "B5", "C1", "C2", "C3"]
    for a in ("A1", "A3"):                      # the ticks kt_late may take: each with every shape of the move
        with_a = {v for s in S.SCENARIOS if a in s["axes"] for v in s["axes"]}
        assert {"B1", "B2", "B5", "C2", "C3"} <= with_a, (a, with_a)


@pytest.mark.parametrize("tuning,tid", list(zip(S.TUNINGS, S.TUNING_IDS)), ids=S.TUNING_IDS)
@pytest.mark.parametrize("s", S.SCENARIOS, ids=S.IDS)
def test_stale_lobby_small_geometry(oracle_cls, s, tuning, tid):
    S.run_scenario(s, tuning, tid, EmuEngineSmall, oracle_cls, **SMALL)


@pytest.mark.parametrize("tuning,tid", PRODUCT_TUNINGS, ids=[t for _, t in PRODUCT_TUNINGS])
@pytest.mark.parametrize("s", S.SCENARIOS, ids=S.IDS)
def test_stale_lobby_product_geometry(oracle_cls, s, tuning, tid):
    """The product's geometry (TT_MIN bystanders and a few), as the device runs it.  Every A1 and A3 tick that the table
    marks for kt_late is claimed, and so confirmed by the counters, under team_late0 = 10^7."""
    claims = S.run_scenario(s, tuning, tid, EmuEngine, oracle_cls, **S.product_size())
    if tid == "late0=1e7":
        want = [k for k, t in enumerate(s["ticks"], 1) if t.get("late")]
        assert [k for k, late in claims if late] == want, (s["name"], claims)


@pytest.mark.parametrize("s", S.SCENARIOS, ids=S.IDS)
def test_stale_lobby_literal(oracle_cls, s):
    S.run_literal(s, oracle_cls)
