#!/usr/bin/env python
"""What mm_rotate (include/mm_wait.h) does to a 1v1 stream (window +-25, region filter, 8 regions, uniform ratings): the
stream of bench.py's cfg-5 leg at 100 000 players/s and a low-rate leg at 500 players/s, 10 ms ticks, real time, with 0, 1
and 4 rounds of rotate-then-tick per period (stream.run_stream's `rotate`; 0 rounds = no rotation, the clock still on so
that the wait figures exist).  Recorded, not asserted: wait p50 / p99 (the engine's own figure, whole periods), tick_cost p50,
matched, rotated, rounds run and whether the leg kept up (its elapsed time against the schedule's).

Usage (GPU box, repo root):  python tools/bench_rotate_stream.py [--seconds 5] > profiles/wait_rotate_stream.json"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def leg(qps, seconds, tick_ms, rounds, seed):
    from microservice_matchmaking_amd import Engine, make_config, mode_1v1
    from microservice_matchmaking_amd.sharding import ShardedSearch
    from microservice_matchmaking_amd.stream import run_stream, stream_batch, stream_schedule
    cfg = make_config([mode_1v1(window=25, region_filter=True)], capacity=1 << 20)
    sched = stream_schedule(qps, seconds, tick_ms, seed)
    batches = [stream_batch(s[2], s[3]) for s in sched]
    with ShardedSearch(cfg, Engine, 0, 1) as sh:
        kw = {"rotate": {"max_seated": [1], "min_queue": 1, "rounds": rounds}} if rounds else {"ttl_ms": 1 << 30}
        res = run_stream(sh, sched, realtime=True, batches=batches, **kw)
        seated = sum(len(sh.engine.lobby_state(0, g)[0]) for g in range(int(cfg.n_groups)))
    w = res["wait_ms"][0]
    pct = lambda a, q: float(np.percentile(a, q)) if a.size else None
    return {"qps": qps, "seconds": seconds, "tick_ms": tick_ms, "rounds": rounds, "arrivals": res["arrivals"],
            "matched": res["matched"], "still_waiting": int(sum(d.sum() for d in res["depth"])) + seated,
            "wait_ms_p50": pct(w, 50), "wait_ms_p99": pct(w, 99),
            "tick_cost_ms_p50": pct(res["tick_cost"] * 1e3, 50), "tick_cost_ms_p99": pct(res["tick_cost"] * 1e3, 99),
            "rotated": res.get("rotated", [0])[0], "rotate_rounds": res.get("rotate_rounds", [0])[0],
            "elapsed_s": res["elapsed"], "kept_up": bool(res["full_at_s"] is None and res["elapsed"] < seconds + 0.05),
            "full_at_s": res["full_at_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--tick-ms", type=float, default=10.0)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU; there is no CPU path"
    from bench import kernel_source_hash
    legs = [leg(qps, args.seconds, args.tick_ms, rounds, 5) for qps in (100_000, 500) for rounds in (0, 1, 4)]
    print(json.dumps({"workload": "1v1 stream, +-25 rating + region filter, 8 regions, uniform ratings, capacity 2^20, real time",
                      "source_hash": kernel_source_hash(), "device": torch.cuda.get_device_name(0), "legs": legs,
                      "note": "rounds 0: no rotation (clock on, a time-out nobody reaches).  wait_ms: clock at the tick minus clock at "
                              "the enqueue, whole periods.  Recorded, not asserted."}, indent=1))


if __name__ == "__main__":
    main()
