"""tests/stale_lobby_scenarios.py on the device, at the product's geometry, under every launch shape: a stored lobby that
a cancel left stale, the anchor's move in every kernel's stored-lobby fill.  A case is one engine and three ticks of
TT_MIN-odd players.  The shim's twin, and the literal restatement, are in tests/test_stale_lobby.py."""
import pytest

import stale_lobby_scenarios as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_cls():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    from microservice_matchmaking_amd import Engine
    return Engine


@pytest.mark.parametrize("tuning,tid", list(zip(S.TUNINGS, S.TUNING_IDS)), ids=S.TUNING_IDS)
@pytest.mark.parametrize("s", S.SCENARIOS, ids=S.IDS)
def test_gpu_stale_lobby(gpu_cls, oracle_cls, s, tuning, tid):
    """Engine vs oracle and the hand-derived literals after every tick; the path counters place every tick the table
    claims for kt_late there (all of the marked ones under team_late0 = 10^7)."""
    claims = S.run_scenario(s, tuning, tid, gpu_cls, oracle_cls, **S.product_size())
    if tid == "late0=1e7":
        want = [k for k, t in enumerate(s["ticks"], 1) if t.get("late")]
        assert [k for k, late in claims if late] == want, (s["name"], claims)
