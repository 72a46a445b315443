"""The sorted route of mm_partners and the rule calls (include/mm_wait.h, mm_tuning.wait_sort_mtests) on the CPU shim: the
partner counts from binary searches in mm_partner_stats' sorted table instead of queries x group length predicate tests.
Results do not change by a word, so the drivers of tests/partners_scenarios.py and tests/move_if_scenarios.py run unchanged on
an engine class forced onto the route (sorted_cls asserts the route after every call), with numpy over the unchanged oracle
as the witness; tests/partners_sorted_scenarios.py adds the shapes at which the new code can go wrong.  The same drivers run
on the GPU in tests/test_gpu_partners_sorted.py."""
import pytest

import move_if_scenarios as mv
import partners_scenarios as ps
from emu_engine import EmuEngine, EmuEngineSmall
from locate_scenarios import chain_lengths
from partners_sorted_scenarios import (empty_table, marked_twin, release_on_failure, role_byte, route_choice, routes_agree,
                                       sorted_cls, table_and_sample, table_lengths)

ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__ if isinstance(c, type) else str(c))


# ---- the existing drivers on the sorted route --------------------------------------------------------------------------

@pytest.mark.parametrize("tick", [True, False], ids=["behind_a_seated_anchor", "no_lobby"])
@pytest.mark.parametrize("n", chain_lengths())
def test_partners_chain_of_exact_length(oracle_cls, n, tick):
    ps.chain_length(sorted_cls(EmuEngine), oracle_cls, n, tick)


@pytest.mark.parametrize("spread", [False, True], ids=["one_group", "seven_groups"])
@pytest.mark.parametrize("nq", ps.query_counts())
def test_partners_query_counts(oracle_cls, nq, spread):
    ps.query_count(sorted_cls(EmuEngine), oracle_cls, nq, spread)


PARTNERS = ["exact_distances", "filters", "self_exclusion", "marks_move_rotate", "seats", "roles", "several_groups", "group_override",
            "none_duplicates_capacity", "null_outputs", "stored_anchor_has_no_partner", "partners_script"]


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("driver", PARTNERS)
def test_partners_driver_on_the_sorted_route(oracle_cls, engine_cls, driver):
    getattr(ps, driver)(sorted_cls(engine_cls), oracle_cls)


@pytest.mark.parametrize("marker", ["cancel", "expire"])
def test_partners_marks(oracle_cls, marker):
    ps.marks(sorted_cls(EmuEngine), oracle_cls, marker)


@pytest.mark.parametrize("tick", [True, False], ids=["behind_a_seated_anchor", "no_lobby"])
@pytest.mark.parametrize("n", chain_lengths())
def test_move_if_chain_of_exact_length(oracle_cls, n, tick):
    mv.chain_length(sorted_cls(EmuEngine), oracle_cls, n, tick)


@pytest.mark.parametrize("spread", [False, True], ids=["one_group", "seven_groups"])
@pytest.mark.parametrize("k1", ps.query_counts())
def test_move_if_candidate_counts(oracle_cls, k1, spread):
    mv.candidate_count(sorted_cls(EmuEngine), oracle_cls, k1, spread)


MOVE_IF = ["limits", "pool_at_entry", "seats", "into_company", "full_on_the_selected", "wrapped_ring", "out_plus_stamped", "move_if_script"]


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("driver", MOVE_IF)
def test_move_if_driver_on_the_sorted_route(oracle_cls, engine_cls, driver):
    getattr(mv, driver)(sorted_cls(engine_cls), oracle_cls)


# ---- the new drivers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", table_lengths())
def test_table_lengths_around_the_sample_and_the_sort_tile(oracle_cls, n):
    table_and_sample(EmuEngine, oracle_cls, n)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_self_comes_off_per_query_a_marked_twin_counts_the_live_one(oracle_cls, engine_cls):
    marked_twin(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_by_role_from_the_role_keyed_table(oracle_cls, engine_cls):
    role_byte(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_an_empty_table(oracle_cls, engine_cls):
    empty_table(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_size_rule_at_its_boundary(oracle_cls, engine_cls):
    route_choice(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_two_routes_agree_on_a_random_script(engine_cls):
    routes_agree(engine_cls)


def test_a_failed_table_allocation_releases_the_scratch_and_leaves_the_engine_usable(oracle_cls):
    release_on_failure(EmuEngine, oracle_cls, EmuEngine.ensure_lib())
