"""Moves, rotations and stamped enqueues in front of the long-chain walks (tests/long_chain_scenarios.py) on the CPU shim's
tiny geometry: the tick behind the call runs the tiled pair path, the team pass kernels on several chunks or kt_late from the
first pass, and every case asserts from mm_path_stats that it did.  The same drivers run at the product's geometry on the GPU
in tests/test_gpu_long_chain.py."""
import pytest

import geometry as G
from emu_engine import EmuEngineSmall
from long_chain_scenarios import (PAIR_LENGTHS, TEAM_TUNING_IDS, TEAM_TUNINGS, long_script, pair_moved_in, pair_rotated, team_moved_in,
                                  stream_long, team_stream_regime_both)


@pytest.fixture(scope="module")
def geo():
    return G.geometry(EmuEngineSmall, small=True)


@pytest.mark.parametrize("wrapped", [False, True], ids=["contiguous", "wrapped"])
@pytest.mark.parametrize("route", ["move", "move_out+stamped"])
@pytest.mark.parametrize("which", sorted(PAIR_LENGTHS))
def test_a_move_into_a_pair_chain_at_the_tiled_paths_threshold(oracle_cls, geo, which, route, wrapped):
    pair_moved_in(EmuEngineSmall, oracle_cls, geo, which, route, wrapped)


@pytest.mark.parametrize("tuning", [None, {"pair_persist": 0}], ids=["kp_rounds", "kp_round"])
def test_a_rotation_in_front_of_a_tiled_pair_tick(oracle_cls, geo, tuning):
    pair_rotated(EmuEngineSmall, oracle_cls, geo, tuning)


@pytest.mark.parametrize("tuning,path_ok", TEAM_TUNINGS, ids=TEAM_TUNING_IDS)
def test_a_move_into_a_team_chain_of_several_chunks(oracle_cls, geo, tuning, path_ok):
    team_moved_in(EmuEngineSmall, oracle_cls, geo, tuning, path_ok)


def test_refused_roles_at_a_count_above_a_bucketing_block(oracle_cls, geo):
    team_moved_in(EmuEngineSmall, oracle_cls, geo, *TEAM_TUNINGS[0], clear=False)


def test_the_low_rate_regime_stays_on_kt_late_behind_rotations_and_moves(oracle_cls, geo):
    team_stream_regime_both(EmuEngineSmall, oracle_cls, geo)


def test_a_stream_with_a_fallback_rule_and_rotations_over_a_team_path_chain_is_the_owner_route(oracle_cls, geo):
    stream_long(EmuEngineSmall, oracle_cls, geo)


@pytest.mark.parametrize("seed,restart_at", [(2, ()), (6, (1,))], ids=["seed2", "seed6-restart"])
def test_random_script_of_every_wait_call_in_front_of_long_chains(oracle_cls, geo, seed, restart_at):
    long_script(EmuEngineSmall, oracle_cls, geo, seed=seed, restart_at=restart_at)
