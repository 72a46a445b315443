"""mm_expire_if, mm_move_if and mm_move_out_if (include/mm_wait.h) on the CPU shim: expiry and moves that select, of the
players old enough, those whose partner count lies in a range.  The reference has neither a time-out nor a view of who fits
whom (requeue_player/5, lib/search/worker.ex:239-248, requeues for ever), and the calls add no matching rule: the selection
is mm_expire's list filtered by mm_partners' number, both with numpy witnesses over the unchanged oracle, and the effect is
the oracle's cancel plus enqueue (tests/move_if_scenarios.py).  The same drivers run on the GPU in tests/test_gpu_move_if.py."""
import ctypes as C

import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from locate_scenarios import chain_lengths
from move_if_scenarios import (allocates_on_first_use, candidate_count, chain_length, errors,
                               full_on_the_selected, into_company, limits, move_if_script, out_plus_stamped, plain_calls,
                               pool_at_entry, seats, sharded, stream_is_the_owner_route, wrapped_ring)
from partners_scenarios import query_counts

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__ if isinstance(c, type) else str(c))


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("tick", [True, False], ids=["behind_a_seated_anchor", "no_lobby"])
@pytest.mark.parametrize("n", chain_lengths())
def test_the_interior_of_a_chain_of_exact_length_is_selected(oracle_cls, engine_cls, n, tick):
    chain_length(engine_cls, oracle_cls, n, tick)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("spread", [False, True], ids=["one_group", "seven_groups"])
@pytest.mark.parametrize("k1", query_counts())
def test_candidate_counts_around_the_tile_of_queries(oracle_cls, engine_cls, k1, spread):
    candidate_count(engine_cls, oracle_cls, k1, spread)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_partner_counts_and_distances_exactly_at_the_limits(oracle_cls, engine_cls):
    limits(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_selection_is_judged_on_the_pool_at_entry(oracle_cls, engine_cls):
    pool_at_entry(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_seats_as_candidates_as_partners_and_refused_roles(oracle_cls, engine_cls):
    seats(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_move_only_where_someone_fits_over_seven_rating_groups(oracle_cls, engine_cls):
    into_company(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_full_is_judged_on_the_selected_not_on_the_old_enough(oracle_cls, engine_cls):
    full_on_the_selected(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_a_wrapped_ring_with_a_waiting_player_in_the_way(oracle_cls, engine_cls):
    wrapped_ring(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_any_partner_count_makes_each_call_its_plain_call(engine_cls):
    plain_calls(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_move_out_if_plus_enqueue_stamped_is_move_if(oracle_cls, engine_cls):
    out_plus_stamped(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_errors(engine_cls):
    errors(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_nothing_is_allocated_before_the_first_call_and_nothing_more_by_a_shorter_one(engine_cls):
    lib = engine_cls.ensure_lib()
    lib.emu_live_blocks.restype = C.c_long
    allocates_on_first_use(engine_cls, lib.emu_live_blocks)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("seed", [1, 2])
def test_random_script_of_every_call_with_drawn_rules(oracle_cls, engine_cls, seed):
    move_if_script(engine_cls, oracle_cls, seed=seed)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_sharded_search_on_one_rank_is_the_engines(engine_cls):
    sharded(engine_cls)


def test_stream_with_a_five_element_fallback_rule_is_the_owner_route(oracle_cls):
    stream_is_the_owner_route(EmuEngineSmall, oracle_cls)
