"""mm_partner_stats (include/mm_wait.h) on the CPU shim: mm_partners' count and gap for every waiting player of a mode,
aggregated per rating group from a radix-sorted table of the candidates (k_fit_* in csrc/mm_wait.inc).  The reference sees a
queue's depth only (Search.Worker.status/0, lib/search/worker.ex:115-117, :326-334); the call changes nothing, so numpy over
the unchanged oracle's lists is the witness for every word, and the engine's own mm_partners over the same slots — the
quadratic route — is a second one (tests/partner_stats_scenarios.py).  The same drivers run on the GPU in
tests/test_gpu_partner_stats.py."""
import ctypes as C
import gc
import os
import subprocess

import pytest

from emu_engine import EmuEngine, EmuEngineSmall
from microservice_matchmaking_amd._abi import MM_PARTNER_HIST, MMPartnerGroup
from partner_stats_scenarios import (all_equal, allocates_on_first_use, bias_and_clamp, errors, out_of_memory, radix_byte, seats_and_roles,
                                     segments, sharded, stats_script, tile_boundary, tile_counts, two_modes, who_waits)
from move_scenarios import four_mode_config
from wait_scenarios import three_mode_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = [EmuEngine, EmuEngineSmall]
ids = dict(ids=lambda c: c.__name__ if isinstance(c, type) else str(c))


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("n", tile_counts())
def test_both_sides_of_the_sort_tile_and_of_the_walks_boundaries(oracle_cls, engine_cls, n):
    tile_boundary(engine_cls, oracle_cls, n)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("n", [1, 2, 65])
def test_short_tables_behind_a_seated_anchor(oracle_cls, engine_cls, n):
    tile_boundary(engine_cls, oracle_cls, n, tick=True)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_every_radix_pass_matters_and_is_stable(oracle_cls, engine_cls, byte):
    radix_byte(engine_cls, oracle_cls, byte)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_all_ratings_equal(oracle_cls, engine_cls):
    all_equal(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_the_bias_and_the_clamp_at_the_ends_of_int32(oracle_cls, engine_cls):
    bias_and_clamp(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_segments_of_group_region_and_party_do_not_see_each_other(oracle_cls, engine_cls):
    segments(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
@pytest.mark.parametrize("cfg_of", [three_mode_config, four_mode_config], ids=["three_modes", "four_modes"])
def test_own_mode_and_another_modes_chains(oracle_cls, engine_cls, cfg_of):
    two_modes(engine_cls, oracle_cls, cfg_of)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_marked_players_do_not_wait(oracle_cls, engine_cls):
    who_waits(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_seats_are_queries_and_candidates(oracle_cls, engine_cls):
    seats_and_roles(engine_cls, oracle_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_errors(engine_cls):
    errors(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_nothing_is_allocated_before_the_first_call_and_the_scratch_grows_with_the_pool(engine_cls):
    lib = engine_cls.ensure_lib()
    lib.emu_live_blocks.restype = C.c_long
    allocates_on_first_use(engine_cls, lib.emu_live_blocks)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_out_of_memory_releases_the_scratch_and_leaves_the_engine_usable(oracle_cls, engine_cls):
    gc.collect()                                           # (engines an earlier test dropped without closing)
    out_of_memory(engine_cls, oracle_cls, engine_cls.ensure_lib())


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_sharded_search_partner_stats_on_one_rank_is_the_engines(engine_cls):
    sharded(engine_cls)


@pytest.mark.parametrize("engine_cls", ENGINES, **ids)
def test_random_script_of_every_call_with_questions_in_between(oracle_cls, engine_cls):
    stats_script(engine_cls, oracle_cls)


def test_the_record_is_304_bytes_in_c_and_in_ctypes(tmp_path):
    probe = ('#include <stdio.h>\n#include <stddef.h>\n#include "mm_wait.h"\nint main(void){printf("%zu %zu %zu %u\\n", '
             'sizeof(mm_partner_group), offsetof(mm_partner_group, partners_sum), offsetof(mm_partner_group, gap_hist), '
             'MM_PARTNER_HIST);return 0;}\n')
    exe = str(tmp_path / "mm_partner_group_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=probe.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [304, MMPartnerGroup.partners_sum.offset, MMPartnerGroup.gap_hist.offset, MM_PARTNER_HIST]
    assert C.sizeof(MMPartnerGroup) == 304
