"""Loads tests/emu/libmm_engine_emu.so — the UNMODIFIED engine source compiled against the
fiber shim (tests/emu/).  Test infrastructure only: exercises kernel control logic on a box
without a GPU.  The product package never loads this library."""
import ctypes as C
import os
import subprocess

from microservice_matchmaking_amd._abi import EngineBase, bind

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def load():
    subprocess.check_call(["make", "-C", _DIR, "--no-print-directory"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.environ.get("MM_EMU_LIB") or os.path.join(_DIR, "libmm_engine_emu.so"))   # see MM_EMU_SMALL_LIB
    return bind(lib, "mm_")


class EmuEngine(EngineBase):
    _prefix = "mm_"
    _load = staticmethod(load)

    def __init__(self, cfg, tuning=None):
        EmuEngine.ensure_lib()
        super().__init__(cfg, tuning)


def load_small():
    subprocess.check_call(["make", "-C", _DIR, "--no-print-directory"], stdout=subprocess.DEVNULL)
    # MM_EMU_SMALL_LIB: another build of the same source (tests/emu_asan_stress.sh: AddressSanitizer)
    lib = C.CDLL(os.environ.get("MM_EMU_SMALL_LIB") or os.path.join(_DIR, "libmm_engine_emu_small.so"))
    return bind(lib, "mm_")


class EmuEngineSmall(EngineBase):
    """Same source built with PK_T=512 / PL_MAX=1536: a few thousand players walk the tiled
    path (tile tables, routing, compaction) and then the LDS-resident kernel."""
    _prefix = "mm_"
    _lib = None

    _load = staticmethod(load_small)

    def __init__(self, cfg, tuning=None):
        EmuEngineSmall.ensure_lib()
        super().__init__(cfg, tuning)
