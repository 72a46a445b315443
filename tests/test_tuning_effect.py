"""Every tuning field reaches the host loops, and none of them changes a result: one engine per knob setting on the CPU
shim (tiny geometry), each against the oracle, its launch counts against tests/golden/tuning_path_stats.json — recorded
by tools/record_tuning_path_stats.py.  Two speed knobs wired to each other's place change no lobby; they change these
counts, or the record mm_tuning_get returns."""
import pytest

from emu_engine import EmuEngineSmall
from tuning_scenarios import SHIM, UNRECORDED, Reference, knob_cases, load_fixture, recorded, run_case

CASES = knob_cases(EmuEngineSmall)


@pytest.fixture(scope="module")
def ref(oracle_cls):
    r = Reference(oracle_cls, SHIM)
    yield r
    r.close()


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_covers_the_knob_list(fixture):
    assert fixture["shape"] == SHIM
    assert sorted(fixture["cases"]) == sorted(cid for cid, t in CASES if not set(t) & set(UNRECORDED))


@pytest.mark.parametrize("cid,tuning", CASES, ids=[c[0] for c in CASES])
def test_one_knob_off_its_default(ref, fixture, cid, tuning):
    got = recorded(run_case(EmuEngineSmall, ref, tuning))
    if not set(tuning) & set(UNRECORDED):
        assert got == fixture["cases"][cid], cid
