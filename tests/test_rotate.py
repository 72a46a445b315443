"""mm_rotate (include/mm_wait.h) on the CPU shim: the players of a short-handed stored lobby leave it and rejoin the tail of
their own queue with the stamps they had, so a chain whose anchor nobody fits moves on.  The reference has one open lobby per
(rating group, mode) and ends a search pass that seats nobody (docs/MATCH_CHECK.md section 4); a rotation is a cancel of the
listed seats plus an enqueue of the same rows, so the unchanged oracle is the witness (tests/rotate_scenarios.py).  The same
drivers run on the GPU in tests/test_gpu_rotate.py."""
import numpy as np
import pytest

from carry_scenarios import spawn
from emu_engine import EmuEngine, EmuEngineSmall
from rotate_scenarios import (LOW_RATE, SHAPES, RotOwnerEngine, assert_ranks_are_one_engine, assert_share, blocked_head,
                              boundaries, dead_seat, errors, full_one_short, group_counts, group_override,
                              host_route_equivalence, lobby_shape, rotate_script, slots_contiguous,
                              slots_wrapped_with_a_waiting_player_in_the_way, stream_one, stream_worker)

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__)


# ---- 1. named cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_blocked_head_rotates_and_the_two_behind_it_meet(oracle_cls, engine_cls):
    blocked_head(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("n_groups", [1, 7, 16])
def test_group_counts_with_empty_lobby_only_and_queue_only_groups(oracle_cls, engine_cls, n_groups):
    with_queue = 1 if n_groups == 1 else sum(g % 4 == 3 for g in range(n_groups))
    lobby_only = 0 if n_groups == 1 else sum(g % 4 == 1 for g in range(n_groups))
    assert group_counts(engine_cls, oracle_cls, n_groups) == [with_queue, with_queue + lobby_only]


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_lobby_shapes(oracle_cls, engine_cls, name):
    assert lobby_shape(engine_cls, oracle_cls, name) == SHAPES[name][3]


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_cancelled_seat_does_not_count_and_is_not_listed(oracle_cls, engine_cls):
    dead_seat(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_max_seated_and_min_queue_boundaries(oracle_cls, engine_cls):
    boundaries(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_new_slots_are_the_plain_range(oracle_cls, engine_cls):
    slots_contiguous(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_new_slots_step_over_a_waiting_player_and_wrap(oracle_cls, engine_cls):
    slots_wrapped_with_a_waiting_player_in_the_way(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_free_slots_one_short_refuse_the_rotation_and_nothing_has_changed(oracle_cls, engine_cls):
    full_one_short(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_player_placed_by_override_stays_in_its_group(oracle_cls, engine_cls):
    group_override(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_host_route_on_a_second_engine_gives_the_same(oracle_cls, engine_cls):
    host_route_equivalence(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_errors_and_nothing_selected(engine_cls):
    errors(engine_cls)


# ---- 2. random scripts ---------------------------------------------------------------------------------------------------

def _script_against_the_restatement(engine_cls, oracle_cls, seed):
    """The restatement first — on the owner route alone (oracle + numpy tables) at least a quarter of the script's rotate
    calls select somebody — then the engine: the same share, and everything the restatement logged."""
    want, calls, hits = rotate_script(RotOwnerEngine, oracle_cls, seed=seed)
    assert_share(calls, hits)
    log, calls, hits = rotate_script(engine_cls, oracle_cls, seed=seed)
    assert_share(calls, hits)
    assert log == want
    return log


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_random_script_seed_1(oracle_cls, engine_cls):
    _script_against_the_restatement(engine_cls, oracle_cls, 1)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_random_script_seed_2_with_a_restart(oracle_cls, engine_cls):
    straight = _script_against_the_restatement(engine_cls, oracle_cls, 2)
    log, calls, hits = rotate_script(engine_cls, oracle_cls, seed=2, restart_at=(2, 5))
    assert_share(calls, hits)
    assert log == straight


# ---- 3. the stream -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def owner_streams(oracle_cls):
    return {r: stream_one(RotOwnerEngine, r) for r in (None, 1, 4)}


def test_stream_without_rotate_is_todays_stream(owner_streams):
    got, want = stream_one(EmuEngineSmall, None), owner_streams[None]
    assert got == want and "rotated" not in got


@pytest.mark.parametrize("rounds", [1, 4])
def test_stream_with_rotation_on_the_shim_is_the_owner_route(owner_streams, rounds):
    want, got = owner_streams[rounds], stream_one(EmuEngineSmall, rounds)
    assert got["digests"] == want["digests"] and got["lobbies"] == want["lobbies"] and got["matched"] == want["matched"]
    assert got["rotated"] == want["rotated"] and got["rotate_rounds"] == want["rotate_rounds"] and got["depth"] == want["depth"]
    assert np.array_equal(got["wait_ms"][0], want["wait_ms"][0])
    assert got["rotated"][0] > 0 and got["matched"] > owner_streams[None]["matched"]
    assert got["rotate_rounds"][0] > owner_streams[1]["rotate_rounds"][0] or rounds == 1


@pytest.mark.parametrize("rounds", [1, 4])
def test_stream_with_rotation_on_two_ranks_is_the_one_engine(owner_streams, rounds):
    gathered = spawn(stream_worker, 2, ("emu", rounds))
    assert all(r["matched"] > 0 for r in gathered)               # both ranks own chains that seat people
    assert_ranks_are_one_engine(gathered, owner_streams[rounds])


def test_low_rate_stream_matches_more_with_rotation(oracle_cls):
    """50 arrivals a second into a region-filtered 1v1, 100 ms periods: the head-of-line blocking of docs/MATCH_CHECK.md
    section 4 leaves most players waiting; one round of rotation a period lets them meet.  First on the restatement."""
    without, with_ = stream_one(RotOwnerEngine, None, LOW_RATE), stream_one(RotOwnerEngine, 1, LOW_RATE)
    print("owner route: matched %d without, %d with rotation" % (without["matched"], with_["matched"]))
    assert with_["matched"] > without["matched"]
    got0, got1 = stream_one(EmuEngine, None, LOW_RATE), stream_one(EmuEngine, 1, LOW_RATE)
    assert got0["matched"] == without["matched"] and got1["matched"] == with_["matched"]
    assert got1["matched"] > got0["matched"] and got1["digests"] == with_["digests"]
