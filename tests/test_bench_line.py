"""bench.py's reporting code without a GPU: (1) the `roofline` arithmetic on the numbers of the
committed MI355X run, (2) a DRY RUN of bench.main() with the engine replaced by the fiber-shim
build of the kernel source (tests/emu/) and torch.cuda stubbed — it checks that the ONE JSON
line the driver parses has every field of the contract and consistent arithmetic.  Nothing here
is a measurement; the numbers a dry run prints are discarded."""
import ctypes as C
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT
from emu_engine import EmuEngine

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_roofline_block_reproduces_the_committed_line():
    with open(os.path.join(ROOT, "profiles", "r01_bench_1m_1v1_final.json")) as f:
        ref = json.loads(f.readline())
    r = bench.roofline_block("1v1", ref["pairs_per_step"], 8, ref["kernel_ms"]["walk"], ref["ms_per_step"],
                             1_000_000, ref["passes_max"], ref["roofline"]["traffic"])
    assert r["achieved"] == pytest.approx(ref["roofline"]["achieved"], rel=1e-9)
    assert r["frac"] == pytest.approx(ref["roofline"]["frac"], rel=1e-9)
    assert r["algorithmic_bytes_per_launch"] == ref["roofline"]["algorithmic_bytes_per_launch"]
    assert r["peak"] == 8000.0 and r["unit"] == "GB/s" and r["bound"] == "hbm"
    # companions of SURVEY.md section 8(d)
    assert r["physical_gbs"] == pytest.approx(ref["roofline"]["traffic"] / (ref["kernel_ms"]["walk"] * 1e-3) / 1e9)
    assert r["compulsory_bytes_per_tick"] == 20e6
    assert r["compulsory_frac"] == pytest.approx(20e6 / (ref["ms_per_step"] * 1e-3) / 8e12)
    assert r["frac_of_measured_copy_peak"] == pytest.approx(r["achieved"] / 6290.0)
    assert r["tile_positions"] == 8192
    none = bench.roofline_block("5v5", 1e6, 12, 0.0, 0.0, 1000, 3, None)
    assert none["achieved"] == 0.0 and none["physical_gbs"] is None and none["tile_positions"] == 512
    assert none["latency_floor_ms"] is None and "traffic_note" not in none
    # the latency ceiling of a one-launch-per-pass design: passes x one dependent kernel boundary
    lat = bench.roofline_block("1v1", 7e7, 8, 16.0, 17.0, 1_000_000, 600, None, boundary_us=1.5, traffic_note="stale")
    assert lat["latency_floor_ms"] == pytest.approx(0.9) and lat["frac_of_latency_ceiling"] == pytest.approx(0.9 / 16.0)
    assert lat["us_per_pass"] == pytest.approx(16000.0 / 600) and lat["traffic_note"] == "stale"


def test_critical_path_model_is_barriers_hops_boundaries_and_lds_steps():
    # the driver's cfg-2 tick of round 4: 336 passes in kp_rounds with 24 hops each, 26 kp_round launches, 270 passes in kp_late
    path = {"paths": 2, "crit_group": 0, "crit_passes": 632, "crit_rounds_passes": 336, "crit_rounds_hops": 336 * 24,
            "crit_round_passes": 26, "crit_late_passes": 270, "crit_late_lobbies": 7300}
    ms, parts = bench.critical_path_ms(path, boundary_us=2.0)
    c = bench.CRIT
    assert parts["kp_rounds"] == pytest.approx((336 * c["barrier_us"] + 336 * 24 * c["hop_l2_us"]) * 1e-3)
    assert parts["kp_round"] == pytest.approx(26 * (2.0 + 24 * c["hop_mem_us"]) * 1e-3)
    assert parts["kp_late"] == pytest.approx((7300 * c["late_step_us"] + 270 * c["late_pass_us"]) * 1e-3)
    assert ms == pytest.approx(sum(parts.values())) and 1.5 < ms < 2.5
    r = bench.roofline_block("1v1", 7e7, 8, 9.6, 10.3, 1_000_000, 632, None, 2.0, None, None, path)
    assert r["frac_of_critical_path"] == pytest.approx(ms / 9.6) and r["latency_floor_ms"] == pytest.approx(632 * 2.0e-3)
    assert bench.critical_path_ms(None) == (None, None) and bench.critical_path_ms({"paths": 4, "crit_passes": 9}) == (None, None)


def test_round6_line_measured_primitives_team_model_and_by_kernel():
    """(c) the pair model's primitives come from the tick's own timers when mm_path_stats has them
    (clock from kp_late's chase, barrier and L2-hit hop from tile 1's walker), (b) the team path has a critical-path model
    of its own (the chaser's boundaries, dependent F loads and look-ups), (a) roofline.by_kernel lists the walk's kernels with
    time and bytes and prices kp_nx_init by SURVEY 8(d)'s convention — labelled, never `frac`."""
    path = {"paths": 2, "crit_group": 0, "crit_passes": 632, "crit_rounds_passes": 336, "crit_rounds_hops": 336 * 24,
            "crit_round_passes": 26, "crit_late_passes": 270, "crit_late_lobbies": 7300,
            "crit_timed_passes": 300, "crit_timed_hops": 7200, "crit_barrier_cycles": 300 * 4400, "crit_hop_cycles": 7200 * 280,
            "clk_cycles": 2_300_000, "clk_wall_ticks": 100_000, "pair_nx_init_ns": 150_000}
    prim, src = bench.measured_primitives(path)
    assert prim["clock_mhz"] == pytest.approx(2300.0) and prim["barrier_us"] == pytest.approx(4400 / 2300.0)
    assert prim["hop_l2_us"] == pytest.approx(280 / 2300.0) and "measured in this run" in src["barrier_us"]
    assert bench.measured_primitives({})[0]["barrier_us"] == bench.CRIT["barrier_us"]          # an older library: the constants
    det = {"by_kernel_profiled": [{"kernel": "kp_rounds<8192u>", "hbm_bytes_per_tick": 1e8, "launches_per_tick": 8, "us_per_tick": 6000.0,
                                    "avg_us_per_launch": 750.0, "gbs": 16.7},
                                   {"kernel": "kp_nx_init", "hbm_bytes_per_tick": 2e7, "launches_per_tick": 1, "us_per_tick": 149.0,
                                    "avg_us_per_launch": 149.0, "gbs": 134.0}]}
    r = bench.roofline_block("1v1", 7e7, 8, 9.6, 10.3, 1_000_000, 632, 8.6e8, 2.0, None, det, path,
                             {"tests_all": 300_000_000, "tests_nx_init": 140_000_000})
    assert r["critical_path_model"]["primitives_us"]["barrier_us"] == pytest.approx(4400 / 2300.0)
    assert r["predicate_tests_physical"] == 300_000_000 and "4.29 x" in r["predicate_tests_note"]
    nx = [k for k in r["by_kernel"] if k["kernel"] == "kp_nx_init"][0]
    assert nx["duration_us_live"] == pytest.approx(150.0) and nx["tested_candidates"] == 140_000_000
    assert nx["equiv_gbs"] == pytest.approx(140e6 * 8 / 150e-6 / 1e9) and "never `frac`" in nx["label"]
    assert nx["equiv_frac_of_hbm_peak"] == pytest.approx(nx["equiv_gbs"] / 8000.0) and r["frac"] < 0.01
    assert r["by_kernel"][0]["kernel"].startswith("kp_rounds") and r["by_kernel"][0]["us_per_tick"] == 6000.0
    # the team path: 32 passes as three launches with 9 000 lobbies by F o F, 78 as kt_fc with 2 700 by F, 23 inside kt_late
    tpath = {"paths": 4, "crit_team_group": 0, "crit_team_passes": 133, "crit_team_f_passes": 32, "crit_team_fc_passes": 78,
             "crit_team_late_passes": 23, "crit_team_f_lobbies": 9000, "crit_team_fc_lobbies": 2700, "crit_team_late_lobbies": 120,
             "crit_team_lookups": 240, "crit_team_late_lookups": 40}
    ms, parts = bench.team_critical_path_ms(tpath, boundary_us=1.6)
    T = bench.TEAM_CRIT
    assert parts["kt_f|kt_f2|kt_chase"] == pytest.approx((32 * 3 * 1.6 + 4500 * T["hop_pulled_us"]) * 1e-3)
    assert parts["kt_fc"] == pytest.approx((78 * 1.6 + 2700 * T["hop_mem_us"]) * 1e-3)
    assert parts["look-ups"] == pytest.approx((240 * 4 + 40 * 3) * T["trip_us"] * 1e-3) and ms == pytest.approx(sum(parts.values()))
    r5 = bench.roofline_block("5v5", 4.5e7, 12, 8.3, 8.6, 1_000_000, 133, None, 1.6, None, None, tpath)
    assert r5["critical_path_ms"] == pytest.approx(ms) and r5["frac_of_critical_path"] == pytest.approx(ms / 8.3)
    assert r5["critical_path_model"]["passes"]["kt_fc"] == 78 and bench.team_critical_path_ms({"paths": 2}) == (None, None)


def test_predict_speedup_is_the_slowest_rank_not_the_load_share():
    # BASELINE cfg-4 as measured on one GPU in round 2: the pool 66.8 ms, its 3M-player chain alone ~55 ms
    assert bench.predict_speedup(66.8, [55.0, 20.0, 0.0, 18.0]) == pytest.approx(66.8 / 55.0)
    assert bench.predict_speedup(10.0, []) is None and bench.predict_speedup(10.0, [0.0]) is None
    assert bench.stream_capacity(100_000, 3.0) == 1 << 20 and bench.stream_capacity(100_000, 60.0) == 1 << 21
    assert bench.stream_key("mixed", 100000, 60.0, 10.0) == "stream/mixed/qps100000/s60/tick10/seed77"


def test_traffic_file_is_refused_when_the_kernel_sources_changed(tmp_path):
    good = {"workload_players": 1000, "mode": "1v1", "walk_hbm_bytes_per_tick": 5.0, "source_hash": bench.kernel_source_hash()}
    p = tmp_path / "t.json"
    p.write_text(json.dumps(good))
    assert bench.load_traffic(str(p), 1000, "1v1") == (5.0, None)
    assert bench.load_traffic(str(p), 2000, "1v1")[0] is None
    p.write_text(json.dumps(dict(good, source_hash="0000")))
    t, why = bench.load_traffic(str(p), 1000, "1v1")
    assert t is None and "other kernel sources" in why
    assert bench.load_traffic(str(tmp_path / "missing.json"), 1000, "1v1")[0] is None


import threading  # noqa: E402

_SHIM_LOCK = threading.Lock()       # the fiber scheduler of the shim is one per process


class DryEngine(EmuEngine):
    """EmuEngine + enqueue_device (under the shim 'device' memory is host memory).  The shim runs
    one kernel at a time, so calls from bench.py's concurrent-pools threads take turns."""

    def reset(self):
        with _SHIM_LOCK:
            return super().reset()

    def tick(self, mode=0, reuse=False):
        with _SHIM_LOCK:
            return super().tick(mode, reuse=reuse)

    def enqueue_device(self, d_rating, d_cons):
        from microservice_matchmaking_amd._abi import MMEnqueueStats
        fn = self._lib.mm_enqueue_device
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(MMEnqueueStats)]
        fn.restype = C.c_int
        first, st = C.c_uint32(), MMEnqueueStats()
        with _SHIM_LOCK:
            rc = fn(self._h, int(d_rating.numel()), C.c_void_p(d_rating.data_ptr()), C.c_void_p(d_cons.data_ptr()),
                    C.byref(first), C.byref(st))
        assert rc == 0
        self.last_enqueue_stats = st.as_dict()
        return int(first.value)


@pytest.mark.parametrize("mode", ["1v1", "5v5"])
def test_bench_main_dry_run_prints_one_contract_line(monkeypatch, mode):
    import torch
    import microservice_matchmaking_amd as pkg
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(pkg, "Engine", DryEngine)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--players", "12000", "--steps", "2", "--warmup", "1", "--mode", mode,
                                      "--stream-seconds", "0.1", "--stream-qps", "20000", "--cpu-baseline-seconds", "0.5",
                                      "--concurrent-pools", "2", "--shared-players", "20000",
                                      "--saturation-qps", "20000", "--saturation-seconds", "0.1"])
    out = io.StringIO()
    with redirect_stdout(out):
        bench.main()
    lines = [ln for ln in out.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith("matched players/sec") and d["unit"] == "matched players/s"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, 2, 1) and d["full"] is True
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(d["matched_fraction"] * 12000 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "physical_gbs", "compulsory_bytes_per_tick",
              "compulsory_frac", "tile_positions", "frac_of_measured_copy_peak"):
        assert k in r, k
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert r["traffic"] is None and "traffic_note" in r   # the PMC figure belongs to the 1M-player workload only
    ex = d["exactness"]                              # the emission digest against the oracle's (committed) digest
    assert ex["ok"] is True and ex["emission_digest"] == ex["oracle_digest"] and ex["key"].startswith(mode + "/12000/")
    # the launch shapes / fall-backs of the last timed tick (mm_path_stats_get), the spread of the timed steps
    assert d["degraded"] is False and d["path"]["paths"] == (2 if mode == "1v1" else 1) and d["path"]["host_looks"] >= 0
    lo, med, hi = d["ms_per_step_min_median_max"]
    assert lo <= med <= hi and lo <= d["ms_per_step"] * 1.0001 and d["n_gpus"] == d["rccl_ranks"] == 1
    for k in ("by_kernel", "predicate_tests_physical", "critical_path_ms", "frac_of_critical_path"):     # round 6: always in the line
        assert k in r, k
    if mode == "1v1":                                # 12000 players: every chain is kp_late's from its first pass
        assert r["predicate_tests_physical"] > d["pairs_per_step"] * 0.5 and "predicate_tests_note" in r
        assert "primitives_source" in r["critical_path_model"] and d["path"]["crit_team_group"] == 0xFFFFFFFF
        assert r["critical_path_ms"] > 0 and r["critical_path_model"]["passes"]["kp_rounds"] == 0
        assert r["critical_path_model"]["passes"]["kp_late"] == d["path"]["crit_passes"] == d["passes_max"]
    else:
        # (3 600 players in the longest chain: below the team path's 4 096, k_walk takes every chain of the dry run's pool)
        assert r["critical_path_ms"] is None and d["path"]["team_f_launches"] + d["path"]["team_fc_launches"] == 0
    assert d["pcie_inclusive"]["value"] > 0 and d["pcie_inclusive"]["steps"] == 2      # the pool handed over in host buffers
    sp = d["shared_pool_n1"]                         # cfg-4's pool on one GPU (here: 20000 players)
    assert sp["exact"] is True and sp["value"] > 0 and "20000 players" in sp["workload"]
    pr = sp["sharding_prediction"]                   # every rank's share of that pool, alone on this GPU
    for nr in ("2", "4", "8"):
        ranks = pr[nr]["per_rank"]
        assert len(ranks) == int(nr) and sum(r["players"] for r in ranks) == 20000
        assert pr[nr]["predicted_speedup"] == pytest.approx(
            sp["ms_per_step"] / max(r["ms_per_step"] for r in ranks))
        assert pr[nr]["load_share_bound"] >= 1.0
    assert [r["players"] for r in pr["8"]["per_rank"]].count(0) == 1          # 7 chains on 8 ranks
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    cp = d["concurrent_pools"]                      # opt-in leg: two engines, two host threads
    assert cp["pools"] == 2 and "error" not in cp and cp["value"] > 0 and cp["steps"] == 2
    if mode == "1v1":
        assert cp["exact_per_pool"] == [True, True] and cp["ok"] is True     # every pool's last tick against the oracle's digest
        sat = d["latency_saturation"]                # the 1v1 stream at rising rates (here: one rate, the dry run's)
        assert [l["enqueue_qps"] for l in sat["legs"]] == [20000] and sat["legs"][0]["exactness"]["ok"] is True
        assert sat["ok"] is True and "highest_sustained_qps" in sat
    if mode == "1v1":
        c3 = d["cfg3"]                               # BASELINE configs[2] beside the headline, checked the same way
        assert c3["exact"] is True and "5v5" in c3["workload"] and c3["value"] > 0 and c3["steps"] >= 2
        assert c3["roofline"]["algorithmic_bytes_per_launch"] == c3["pairs_per_step"] * 12
        assert c3["exactness"]["key"].startswith("5v5/12000/")
        for leg in ("latency", "latency_mixed"):
            assert d[leg]["ok"] is True and d[leg]["emission_digest"] == d[leg]["oracle_digest"]   # vs the committed oracle run
            assert d[leg]["capacity_exhausted_at_s"] is None and d[leg]["tick_cost_ms_max"] >= d[leg]["tick_cost_ms_p50"]
            assert d[leg]["tick_cost_ms_by_10s"][0]["from_s"] == 0.0
            assert d[leg]["p99_ms"] >= d[leg]["p50_ms"] >= 0 and d[leg]["enqueue_qps"] == 20000
            assert d[leg]["floor_p99_ms"] >= d[leg]["floor_p50_ms"] >= 0     # the arrival-limited floor beside it
            assert len(d[leg]["emission_digest"]) == 32
        assert set(np.asarray([len(d["latency_mixed"]["per_mode"])])) == {2}


class CountingDryEngine(DryEngine):
    ticks = 0

    def tick(self, mode=0, reuse=False):
        CountingDryEngine.ticks += 1
        return super().tick(mode, reuse=reuse)


@pytest.mark.parametrize("mode", ["1v1", "5v5"])
def test_bench_plain_run_is_the_headline_alone_and_dumps_its_outputs(monkeypatch, tmp_path, mode):
    """A plain run (no --full): warm-up + --steps ticks and nothing else, the contract fields, no leg beside the headline;
    --dump-outputs writes the last timed step's match list, and a second run with the same pool writes the same arrays."""
    import torch
    import microservice_matchmaking_amd as pkg
    from microservice_matchmaking_amd.sharding import tick_digests, union_digest
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(pkg, "Engine", CountingDryEngine)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)

    def run(steps, warmup, out_dir):
        CountingDryEngine.ticks = 0
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--players", "12000", "--steps", str(steps), "--warmup",
                                          str(warmup), "--mode", mode, "--dump-outputs", str(out_dir)])
        out = io.StringIO()
        with redirect_stdout(out):
            bench.main()
        lines = [ln for ln in out.getvalue().splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        assert CountingDryEngine.ticks == steps + warmup
        return json.loads(lines[0])

    d = run(3, 2, tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "exactness", "roofline"):
        assert k in d, k
    assert (d["steps"], d["warmup"], d["full"]) == (3, 2, False) and d["ms_per_step"] > 0
    assert d["metric"].startswith("matched players/sec") and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] == pytest.approx(d["matched_fraction"] * 12000 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    for leg in ("cpu_baseline", "cfg3", "pcie_inclusive", "shared_pool_n1", "concurrent_pools", "latency",
                "latency_saturation", "latency_mixed", "weak_scaling"):
        assert leg not in d, leg
    assert d["roofline"]["boundary_us"] is None and d["roofline"]["predicate_tests_physical"] is None
    assert d["exactness"]["ok"] is True
    names = ("slots", "players", "score", "group", "pass", "rows")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES_MAX
    lobbies, L = a["slots"].shape
    assert L == (2 if mode == "1v1" else 10) and a["players"].shape == (lobbies, L)
    assert len(a["score"]) == len(a["group"]) == len(a["pass"]) == len(a["rows"]) == lobbies
    assert np.array_equal(a["rows"], np.arange(lobbies)) and a["players"].size == round(d["matched_fraction"] * 12000)
    # the arrays are the list the line's emission digest was taken over
    assert union_digest(tick_digests(0, 7, a["players"].astype(np.int64), a["group"].astype(np.uint32))) == \
        d["exactness"]["emission_digest"]
    run(2, 1, tmp_path / "b")
    for n in names:
        assert np.array_equal(np.load(tmp_path / "b" / (n + ".npy")), a[n]), n


def test_bench_dump_outputs_samples_a_large_list_within_its_budget(tmp_path):
    """A match list larger than the budget: a fixed, seeded sample of lobbies, the same rows in every array; per rank at N > 1."""
    from microservice_matchmaking_amd._abi import Matches
    n, L = 50_000, 2
    rng = np.random.default_rng(3)
    m = Matches(rng.integers(0, 1 << 20, (n, L)).astype(np.uint32), rng.random(n).astype(np.float32),
                rng.integers(0, 7, n).astype(np.uint32), rng.integers(0, 500, n).astype(np.uint32), {})
    ids = m.slots.astype(np.int64) + 7
    budget = 200_000
    p1 = bench.dump_outputs(str(tmp_path / "a"), m, ids, budget=budget)
    p2 = bench.dump_outputs(str(tmp_path / "b"), m, ids, budget=budget)
    a = {k: np.load(v) for k, v in p1.items()}
    assert sum(x.nbytes for x in a.values()) <= budget and 0 < len(a["rows"]) < n
    rows = a["rows"].astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(a["slots"], m.slots[rows]) and np.array_equal(a["players"], ids[rows].astype(np.float64))
    assert np.array_equal(a["score"], m.score[rows]) and np.array_equal(a["pass"], m.pass_[rows])
    for k, v in p2.items():
        assert np.array_equal(np.load(v), a[k]), k
    p3 = bench.dump_outputs(str(tmp_path / "c"), None, None, rank=7, world=8, budget=budget)
    assert os.path.basename(p3["slots"]) == "slots_rank7.npy" and np.load(p3["players"]).size == 0


@pytest.mark.parametrize("world", [2, 8])
def test_bench_ranks_dry_run_shards_one_pool(world, oracle_cls):
    """`bench.py --gpus N` as the driver launches it (one process per rank, env rendezvous on
    127.0.0.1), with gloo standing in for RCCL: rank 0 prints the only line; the workload is ONE
    pool sharded by chain (BASELINE cfg-4's shape), value = players matched by ALL ranks over the
    slowest rank's time, and the union of the ranks' emission lists has the oracle's digest.
    world 8: seven chains on eight ranks, one rank idles and still takes part in the barriers."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_dryrun_worker.py")
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",   # the shim has one device
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, "--full", "--gpus", str(world), "--players", "12000", "--steps", "2",
                                       "--warmup", "1", "--weak-players", "6000", "--stream-seconds", "0.1",
                                       "--stream-qps", "20000"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e.decode()[-2000:]
    lines0 = [ln for ln in outs[0][0].decode().splitlines() if ln.startswith("{")]
    assert len(lines0) == 1
    for o, _ in outs[1:]:
        assert not [ln for ln in o.decode().splitlines() if ln.startswith("{")]
    d = json.loads(lines0[0])
    assert d["n_gpus"] == world and d["scaling"] == "strong"
    assert "sharded across %dxMI355X" % world in d["config"]["workload"] and "12000 players" in d["config"]["workload"]
    assert "cpu_baseline" not in d and "latency" not in d            # rank 0 at N=1 only
    sh = d["config"]["sharding"]
    assert sh["key"] == "(game mode, rating group)" and "none" in sh["collective"] and "no_halo_allgather" in sh
    assert len(sh["per_rank"]) == world and sum(p["players"] for p in sh["per_rank"]) == 12000
    assert sh["idle_ranks"] == ([7] if world == 8 else [])
    for r in sh["idle_ranks"]:
        assert sh["per_rank"][r]["players"] == 0 and sh["per_rank"][r]["matched_players"] == 0
    # every rank's players are in `value`; the slowest rank's clock is the pool's
    assert d["matched_fraction"] * 12000 == pytest.approx(sum(p["matched_players"] for p in sh["per_rank"]))
    assert d["ms_per_step"] == pytest.approx(max(p["ms_per_step"] for p in sh["per_rank"]))
    assert d["value"] == pytest.approx(d["matched_fraction"] * 12000 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    ex = d["exactness"]
    assert ex["ok"] is True and ex["emission_digest"] == ex["oracle_digest"]
    assert d["weak_scaling"]["pool_per_gpu"] == 6000 and d["weak_scaling"]["value"] > 0
    # the speed-up is computed from the gathered per-rank records and rank 0's run of the whole pool
    assert sh["load_share_bound"] >= 1.0 and "speedup_bound" not in sh
    assert sh["speedup_vs_one_gpu"] == pytest.approx(
        bench.predict_speedup(sh["one_gpu_ms_per_step"], [p["ms_per_step"] for p in sh["per_rank"]]))
    lm = d["latency_mixed"]                                           # cfg-5: the two-mode stream, chains over the ranks
    assert lm["ranks"] == world and lm["sharding"]["idle_ranks"] == [] and len(lm["per_mode"]) == 2
    assert lm["ok"] is True and lm["emission_digest"] == lm["oracle_digest"]       # against the committed oracle run
    # the stream's emission on N ranks is the single oracle engine's
    from microservice_matchmaking_amd.config import make_config, mode_1v1, mode_team
    from microservice_matchmaking_amd.sharding import ShardedSearch, union_digest
    from microservice_matchmaking_amd.stream import run_stream, stream_schedule
    from microservice_matchmaking_amd.synth import ROLE_WEIGHTS_5V5
    cfg = make_config([mode_1v1(window=25, region_filter=True), mode_team(5, 2, 50, (1, 1, 1, 1, 1))], capacity=1 << 20)
    with ShardedSearch(cfg, oracle_cls, 0, 1) as one:
        ref = run_stream(one, stream_schedule(20000, 0.1, 10.0, 77), mode_weights=(70, 30),
                         role_weights=ROLE_WEIGHTS_5V5, realtime=False)
    assert lm["emission_digest"] == union_digest(ref["digests"])


def _dry_cmd(*argv):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_dryrun_worker.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return [sys.executable, worker] + list(argv), env


def test_bench_gpus_n_as_one_command_starts_its_own_ranks():
    """`python bench.py --gpus 2 ...` launched as ONE command with no WORLD_SIZE (the shape of the driver's N = 1 command
    with another N): bench.py starts the two ranks itself, the line says n_gpus 2 and the collective saw two ranks —
    it can no longer print an N = 1 number under an `--gpus N` flag ("What's weak" 7)."""
    import subprocess
    cmd, env = _dry_cmd("--gpus", "2", "--players", "12000", "--steps", "2", "--warmup", "1", "--no-secondary", "--no-stream")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and "bench.py itself" in d["launched_by"]
    assert len(d["config"]["sharding"]["per_rank"]) == 2 and d["exactness"]["ok"] is True


def test_bench_force_dist_runs_the_collective_branch_on_one_rank():
    """`--force-dist` (round 6): N = 1 with the process group up — the barriers, the all-reduce of ones and the gathers of the
    N > 1 branch execute on one rank (here over gloo and the shim engine; on the device over RCCL:
    test_gpu_bench_rccl_branch_on_one_rank, which is what found RCCL's banner on stdout)."""
    import subprocess
    cmd, env = _dry_cmd("--force-dist", "--players", "12000", "--steps", "2", "--warmup", "1", "--no-secondary", "--no-stream",
                        "--no-cpu-baseline")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["collective_backend"] != "none" and d["exactness"]["ok"] is True


def test_bench_refuses_a_world_that_is_not_gpus():
    """WORLD_SIZE set by a launcher and different from --gpus: non-zero exit, no line."""
    import subprocess
    cmd, env = _dry_cmd("--gpus", "8", "--players", "12000", "--steps", "1", "--warmup", "0")
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 2 and b"WORLD_SIZE=1" in p.stderr
    assert not [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]


def test_graft_entry_smoke_dry_run(monkeypatch, capsys):
    """__graft_entry__.smoke() with the shim engine: the driver's pre-bench check is runnable code."""
    import torch
    import microservice_matchmaking_amd as pkg
    import __graft_entry__ as entry
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(pkg, "Engine", DryEngine)
    entry.smoke()
    out = capsys.readouterr().out
    assert out.count("smoke ok") == 2


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_gpu_bench_two_ranks_on_one_device():
    """`python bench.py --gpus 2 --same-device` on the box's one GPU (round 6): the N > 1 branch of the bench line with real
    HIP engines in two processes — cfg-4's seeded 10M pool sharded by chain, gloo for the barriers and gathers (two RCCL
    ranks cannot share a device), the union digest = the committed oracle digest.  Not a scaling number and the line says
    so (`same_device`); what it proves is that the branch the driver runs on an 8-GPU node executes."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--same-device", "--steps", "2", "--warmup", "1",
                        "--no-secondary", "--no-stream"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines                   # ONE line on stdout, nothing else (gloo's own chatter goes to stderr)
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["same_device"] is True and d["collective_backend"] == "gloo"
    assert "10000000 players" in d["config"]["workload"]
    sh = d["config"]["sharding"]
    assert len(sh["per_rank"]) == 2 and sum(p_["players"] for p_ in sh["per_rank"]) == 10_000_000
    assert d["exactness"]["ok"] is True and d["exactness"]["emission_digest"] == d["exactness"]["oracle_digest"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_gpu_bench_rccl_branch_on_one_rank():
    """`python bench.py --force-dist` (round 6): the process group of the N > 1 branch with the backend the driver's 8-GPU run
    uses — `nccl` = RCCL — initialised on the box's one GPU, world size 1: communicator creation, the all-reduce of ones on
    the device, every barrier of the timed region and the gathers run for real.  What it cannot show is a second rank:
    no multi-GPU node was available to any round."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--force-dist", "--steps", "3", "--warmup", "1",
                        "--no-secondary", "--no-stream", "--no-cpu-baseline"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["rccl_ranks"] == 1 and d["collective_backend"] == "nccl (RCCL)" and d["same_device"] is False
    assert d["exactness"]["ok"] is True and d["value"] > 5e7
