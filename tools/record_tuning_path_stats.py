#!/usr/bin/env python
"""Records tests/golden/tuning_path_stats.json: the deterministic mm_path_stats fields of tests/tuning_scenarios.py's
two ticks on the CPU shim (tiny geometry), for every knob setting of its list.  Usage: python tools/record_tuning_path_stats.py [out.json]
Run it twice and compare: what does not reproduce does not belong in the record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from emu_engine import EmuEngineSmall  # noqa: E402
from oracle.oracle import OracleEngine, build  # noqa: E402
from tuning_scenarios import FIXTURE, SHIM, STAT_FIELDS, UNRECORDED, Reference, knob_cases, recorded, run_case  # noqa: E402


def main(out):
    build()
    ref = Reference(OracleEngine, SHIM)
    cases = {}
    for cid, tuning in knob_cases(EmuEngineSmall):
        if set(tuning) & set(UNRECORDED):
            continue
        cases[cid] = recorded(run_case(EmuEngineSmall, ref, tuning))
    ref.close()
    doc = {"comment": "mm_path_stats of the 1v1 tick, then of the 5v5 tick, per knob setting; libmm_engine_emu_small.so. "
                      "Not recorded: %s (its kp_rounds launches stop on wall time)." % ", ".join(UNRECORDED),
           "shape": SHIM, "fields": list(STAT_FIELDS), "cases": cases}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
