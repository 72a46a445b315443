"""One knob at a time: the scenario tests/test_tuning_effect.py (CPU shim, tiny geometry) and
tests/test_gpu_tuning_effect.py (device) run for every field of mm_tuning that tests/stress.py draws, and that
tools/record_tuning_path_stats.py records the shim's launch counts of.  A 1v1 chain long enough for the tiled rounds and
a 5v5 chain long enough for the team path, both in one rating group, one tick each; the oracle walks them once and every
engine — whatever its tuning — must emit what it emitted."""
import json
import os

import numpy as np

from helpers import assert_same_state, assert_same_tick
from microservice_matchmaking_amd._abi import cons_make
from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
from stress import COMMON_KNOBS, PAIR_KNOBS, TEAM_KNOBS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tuning_path_stats.json")
# mm_path_stats fields that are a function of the pool and the tuning alone (no clock, no address, no scheduling)
STAT_FIELDS = ("paths", "host_looks", "pair_rounds_launches", "pair_round_launches", "pair_tiled_passes", "pair_rounds_passes",
               "pair_stops_inject", "pair_persist_off", "team_f_launches", "team_fc_launches", "team_late_launches",
               "team_build_launches", "crit_passes", "crit_rounds_passes", "crit_round_passes", "crit_late_passes",
               "crit_team_passes", "crit_team_f_passes", "crit_team_fc_passes", "crit_team_late_passes")
UNRECORDED = ("pair_ptimeout_us",)      # its kp_rounds launches stop on wall time: parity and tuning() only
SHIM = dict(n_pair=2500, n_team=600, capacity=4096)        # five tiles of 512 (PL_MAX 1536); TT_MIN 64
DEVICE = dict(n_pair=20000, n_team=6000, capacity=32768)   # ten tiles of 2048 (PL_MAX 16384); TT_MIN 4096


def knob_cases(engine_cls):
    """[(id, {field: value})]: the defaults, force_generic, and every drawn field at the first and the last value of its
    menu that is not the default of this build."""
    dflt = engine_cls.tuning_defaults()
    cases = [("defaults", {}), ("force_generic=1", {"force_generic": 1})]
    for table in (PAIR_KNOBS, TEAM_KNOBS, COMMON_KNOBS):
        for name, menu in table.items():
            off = [int(v) for v in menu if int(v) != dflt[name]]
            for v in dict.fromkeys((off[0], off[-1])):
                cases.append(("%s=%d" % (name, v), {name: v}))
    return cases


def config(shape):
    return make_config([mode_1v1(window=30), mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=shape["capacity"], timing=False)


def pools(shape):
    r1, r5 = np.random.default_rng([20260, 1]), np.random.default_rng([20260, 5])
    n1, n5 = shape["n_pair"], shape["n_team"]
    return ((r1.integers(0, 1400, size=n1).astype(np.int32), cons_make(0, 0, 0, np.zeros(n1, np.uint32))),
            (r5.integers(0, 1400, size=n5).astype(np.int32), cons_make(1, 0, 0, r5.integers(0, 5, size=n5))))


class Reference:
    """The oracle's two ticks, walked once; its engine stays open for the state comparison."""

    def __init__(self, oracle_cls, shape):
        self.shape, self.cfg = shape, config(shape)
        self.engine = oracle_cls(self.cfg)
        self.slots = [self.engine.enqueue(*p) for p in pools(shape)]
        self.ticks = [self.engine.tick(0), self.engine.tick(1)]
        assert len(self.ticks[0]) > shape["n_pair"] // 8 and len(self.ticks[1]) > shape["n_team"] // 100

    def close(self):
        self.engine.close()


def run_case(engine_cls, ref, tuning):
    """Engine with `tuning` against the reference: lobbies, order, passes, counters, queue order, the tuning record.
    -> [path_stats after the 1v1 tick, after the 5v5 tick]."""
    want = dict(engine_cls.tuning_defaults(), **tuning)
    stats = []
    with (engine_cls(ref.cfg, tuning) if tuning else engine_cls(ref.cfg)) as e:
        assert e.tuning() == want
        for p, s in zip(pools(ref.shape), ref.slots):
            assert np.array_equal(e.enqueue(*p), s)
        for mode in (0, 1):
            assert_same_tick(e.tick(mode), ref.ticks[mode], "%s mode %d" % (tuning, mode))
            stats.append(e.path_stats())
        assert_same_state(e, ref.engine, ref.cfg, str(tuning))
        assert e.tuning() == want
    return stats


def recorded(stats):
    return [{k: int(s[k]) for k in STAT_FIELDS} for s in stats]


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
