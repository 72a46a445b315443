"""mm_partners (include/mm_wait.h) on the CPU shim: how many waiting players of a rating group fit a queried player at a
window and a set of filters — step 2 of match_check (docs/MATCH_CHECK.md) with the queried player in the anchor's place —
split by role, and the distance to the nearest one.  The reference sees a queue's depth only (Search.Worker.status/0,
lib/search/worker.ex:115-117, :326-334); the call changes nothing, so numpy over the unchanged oracle's queue_slots and
lobby_state is the witness for every word (tests/partners_scenarios.py).  The same drivers run on the GPU in
tests/test_gpu_partners.py."""
import ctypes as C

import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from partners_scenarios import (allocates_on_first_use, chain_length, chain_lengths, errors, exact_distances, filters,
                                group_override, marks, marks_move_rotate, none_duplicates_capacity, null_outputs,
                                partners_script, query_count, query_counts, roles, seats, self_exclusion, several_groups,
                                sharded, stored_anchor_has_no_partner)

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__ if isinstance(c, type) else str(c))


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("tick", [True, False], ids=["behind_a_seated_anchor", "no_lobby"])
@pytest.mark.parametrize("n", chain_lengths())
def test_both_sides_of_every_boundary_of_a_chain_of_exact_length(oracle_cls, engine_cls, n, tick):
    chain_length(engine_cls, oracle_cls, n, tick)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("spread", [False, True], ids=["one_group", "seven_groups"])
@pytest.mark.parametrize("nq", query_counts())
def test_query_counts_around_the_tile_of_queries(oracle_cls, engine_cls, nq, spread):
    query_count(engine_cls, oracle_cls, nq, spread)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_partners_at_exactly_the_window_and_the_ends_of_int32(oracle_cls, engine_cls):
    exact_distances(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_each_filter_alone_both_and_none(oracle_cls, engine_cls):
    filters(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_player_is_never_its_own_partner(oracle_cls, engine_cls):
    self_exclusion(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("marker", ["cancel", "expire"])
def test_marked_candidates_are_not_counted_and_marked_queries_are_answered(oracle_cls, engine_cls, marker):
    marks(engine_cls, oracle_cls, marker)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_moved_and_rotated_players_count_where_they_wait_now(oracle_cls, engine_cls):
    marks_move_rotate(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_seats_as_queries_and_as_candidates(oracle_cls, engine_cls):
    seats(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_by_role_with_missing_and_scarce_roles(oracle_cls, engine_cls):
    roles(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_another_modes_chains_across_seven_rating_groups(oracle_cls, engine_cls):
    several_groups(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_player_placed_by_override_is_asked_about_the_group_it_sits_in(oracle_cls, engine_cls):
    group_override(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_none_duplicates_and_slots_past_the_capacity(oracle_cls, engine_cls):
    none_duplicates_capacity(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_any_subset_of_the_outputs_may_be_null_and_the_clock_stays_off(oracle_cls, engine_cls):
    null_outputs(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_errors(engine_cls):
    errors(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_nothing_is_allocated_before_the_first_call_and_nothing_more_by_a_shorter_one(engine_cls):
    lib = engine_cls.ensure_lib()
    lib.emu_live_blocks.restype = C.c_long
    allocates_on_first_use(engine_cls, lib.emu_live_blocks)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_seat_of_a_stored_1v1_lobby_has_no_partner_after_the_tick(oracle_cls, engine_cls):
    stored_anchor_has_no_partner(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_random_script_of_every_call_with_questions_in_between(oracle_cls, engine_cls):
    partners_script(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_sharded_search_partners_on_one_rank_is_the_engines(engine_cls):
    sharded(engine_cls)
