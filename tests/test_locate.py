"""mm_locate (include/mm_wait.h) on the CPU shim: where a slot stands in a mode — queue or stored lobby, rating group,
position, the waiting players ahead, its age, whether a cancel or an expiry has marked it — answered on the device in one
pass of mm_expire's walk.  The reference sees a queue's depth only (Search.Worker.status/0, lib/search/worker.ex:115-117,
:326-334); the call changes nothing, so the unchanged oracle's queue_slots and lobby_state are the witness for every word
(tests/locate_scenarios.py).  The same drivers run on the GPU in tests/test_gpu_locate.py."""
import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from locate_scenarios import (chain_length, chain_lengths, clock_off, clock_on, duplicates, errors, lobby_seats, marks,
                              marks_rotate, no_scratch_leak, none_cases, null_outputs, several_groups, sharded)

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__ if isinstance(c, type) else str(c))


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("tick", [True, False], ids=["behind_a_seated_anchor", "no_lobby"])
@pytest.mark.parametrize("n", chain_lengths())
def test_every_entry_of_a_chain_of_exact_length(oracle_cls, engine_cls, n, tick):
    chain_length(engine_cls, oracle_cls, n, tick)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("marker", ["cancel", "expire"])
def test_marked_entries_keep_their_place_until_the_tick_and_are_gone_after_it(oracle_cls, engine_cls, marker):
    marks(engine_cls, oracle_cls, marker)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_rotated_seat_is_marked_and_its_player_stands_at_the_tail_with_its_age(oracle_cls, engine_cls):
    marks_rotate(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_seats_of_a_short_lobby_in_lobby_states_order(oracle_cls, engine_cls):
    lobby_seats(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_one_query_across_seven_rating_groups(oracle_cls, engine_cls):
    several_groups(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_matched_unused_out_of_range_and_other_mode_slots_are_none(oracle_cls, engine_cls):
    none_cases(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_slot_queried_three_times_gets_three_identical_answers(oracle_cls, engine_cls):
    duplicates(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_no_scratch_is_left_behind_by_slots_that_were_not_found(oracle_cls, engine_cls):
    no_scratch_leak(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_with_the_clock_off_ages_are_zero_and_the_clock_stays_off(oracle_cls, engine_cls):
    clock_off(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_ages_of_players_from_three_stamps(oracle_cls, engine_cls):
    clock_on(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_any_subset_of_the_output_pointers_may_be_null(oracle_cls, engine_cls):
    null_outputs(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_errors(engine_cls):
    errors(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_sharded_search_locate_on_one_rank_is_the_engines(engine_cls):
    sharded(engine_cls)
