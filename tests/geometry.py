"""The walk's geometry, read from the source: every length and distance at which the pair (mm_pair.inc) and team
(mm_team.inc) kernels or their host loop (mm_engine.hip) change behaviour, for the product build and for the
tiny-geometry build of tests/emu (its -D overrides are parsed from tests/emu/Makefile).  The constants come from the
#define lines, the two numbers the host code holds as literals (kp_nx_init's first segment length, kp_init's workgroup)
from the statements that hold them; whatever is renamed or removed makes geometry() raise, so tests/test_boundaries.py
fails instead of testing nothing.  The only number written down here is the wave of 64 lanes.  The tuning defaults that
move boundaries come from the engine class (mm_tuning_default)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "microservice_matchmaking_amd", "csrc")
SOURCES = ("mm_pair.inc", "mm_team.inc", "mm_engine.hip")
EMU_MAKEFILE = os.path.join(HERE, "emu", "Makefile")
EMU_SMALL_TARGET = "libmm_engine_emu_small.so"

CONSTANTS = ("PK_T", "PK_TILES_MAX", "PK_GROUP_MIN", "PK_GS", "PL_MAX", "PL_COMPACT_MIN", "NXI_SEG", "NXI_STAGE", "NX_NONE",
             "NX_FAR", "TT_MIN", "TT_MAX", "TT_CH", "TT_SCAN_CAP", "TF_PAD", "TF_FAR_BITS", "TF_BW", "TL_BITS_MAX",
             "MM_RESULTS_MIN_PAIR", "MM_RESULTS_MIN_TEAM")
TUNING = ("pair_ptiles", "pair_tiles_max", "pair_group_min", "team_cap")
# literals of mm_engine.hip's pair_open that have no #define: name -> the statement that holds the number
HOST_LITERALS = {
    "NX_SEG_MIN": r"uint32_t seg = (\d+)u, stage = NXI_STAGE;",              # kp_nx_init's anchors per workgroup start here and double up to NXI_SEG
    "KP_INIT_ROW": r"hipLaunchKernelGGL\(kp_init, dim3\(G\), dim3\((\d+)\)",   # threads of the workgroup that reads the queue, eight rows unrolled
}
WAVE = 64

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+([A-Za-z_]\w*)[ \t]+(.+?)[ \t]*(?://.*)?$", re.M)


def source_defines():
    """name -> the text of its (object-like) #define, first definition wins, over the three engine sources."""
    out = {}
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            for k, v in _DEFINE.findall(f.read()):
                out.setdefault(k, v)
    return out


def makefile_overrides(target=EMU_SMALL_TARGET, makefile=EMU_MAKEFILE):
    """The -DNAME=value options of one target's recipe in tests/emu/Makefile, the Makefile's own variables expanded."""
    with open(makefile) as f:
        text = f.read().replace("\\\n", " ")
    variables = dict(re.findall(r"^([A-Za-z_]\w*)[ \t]*\??=[ \t]*(.*)$", text, re.M))
    for _ in range(8):                                                       # (variables that hold variables)
        text = re.sub(r"\$\((\w+)\)", lambda m: variables.get(m.group(1), m.group(0)), text)
    m = re.search(r"^%s:.*\n((?:\t.*\n?)+)" % re.escape(target), text, re.M)
    if not m:
        raise KeyError("no target %s in %s" % (target, makefile))
    over = dict(re.findall(r"-D([A-Za-z]\w*)=(\S+)", m.group(1)))           # (not the toolchain's own: -D_FORTIFY_SOURCE)
    if not over:
        raise KeyError("the recipe of %s in %s holds no -D option: not the tiny geometry" % (target, makefile))
    return over


def _value(name, texts, seen=()):
    if name in seen:
        raise ValueError("circular #define: %s" % name)
    if name not in texts:
        raise KeyError("geometry constant %s is not #defined in %s" % (name, ", ".join(SOURCES)))
    expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uU]?[lL]{0,2}\b", r"\1", texts[name])
    expr = re.sub(r"(?<![0-9A-Za-z_])[A-Za-z_]\w*", lambda m: str(_value(m.group(0), texts, seen + (name,))), expr)
    if not re.fullmatch(r"[0-9a-fA-FxX\s()+\-*/<>]+", expr):
        raise ValueError("cannot evaluate #define %s %s" % (name, texts[name]))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def geometry(engine_cls=None, small=False, tuning=None):
    """The geometry of one engine build as a dict: CONSTANTS from the source (with the small build's -D overrides laid
    over them), TUNING from engine_cls.tuning_defaults() with `tuning` (a drawn {field: value}) laid over that."""
    texts = source_defines()
    if small:
        over = makefile_overrides()
        unknown = sorted(set(over) - set(texts))
        if unknown:
            raise KeyError("tests/emu/Makefile overrides what the source does not define: %s" % unknown)
        texts.update(over)
    geo = {name: _value(name, texts) for name in CONSTANTS}
    with open(os.path.join(CSRC, "mm_engine.hip")) as f:
        host = f.read()
    for name, pattern in HOST_LITERALS.items():
        m = re.search(pattern, host)
        if not m:
            raise KeyError("mm_engine.hip no longer holds the statement %s is read from: %s" % (name, pattern))
        geo[name] = int(m.group(1))
    if engine_cls is not None:
        dflt = engine_cls.tuning_defaults()               # (loads the class's library; no engine, no device)
        for name in TUNING:
            geo[name] = int(dflt[name])                   # KeyError: the field was renamed
        for name, v in (tuning or {}).items():
            if name in TUNING:
                geo[name] = int(v)
    geo["small"] = bool(small)
    geo["tile_lengths"] = (geo["PK_T"], geo["PK_T"] // 2, geo["PK_T"] // 4)
    return geo


def tiles_cap(geo):
    """pair_walk: the tile count that chooses the tile length of a batch (kp_rounds on: the smaller of the two knobs)."""
    return min(geo["pair_ptiles"], geo["pair_tiles_max"])


def nx_segs(geo):
    out, s = [], geo["NX_SEG_MIN"]
    while s <= geo["NXI_SEG"]:
        out.append(s)
        s <<= 1
    return out


# Entries of the tables: (B, name, plus, gpu_only).  `plus`: B + 1 is a length of its own (the branch is `<` / `<=` on
# this very number, or a count of tiles rounds up there); without it {B - 1, B} say everything.  `gpu_only`: the CPU shim
# does not run it — the 16-bit codes of nx16, which the small build does not scale (team_boundaries: chains of 2^19 and more).
def _table(rows, geo):
    by = {}
    for b, name, plus in rows:
        e = by.setdefault(int(b), [[], False])
        e[0].append(name)
        e[1] = e[1] or plus
    return [(b, "+".join(n), plus, b >= geo["NX_FAR"]) for b, (n, plus) in sorted(by.items())]


def pair_boundaries(geo):
    """Sorted, de-duplicated chain lengths at which the pair path switches: [(B, name, plus, gpu_only)]."""
    T = geo["tile_lengths"]
    # (PL_MAX, the rows and the segments are `<` / `>=` tests: B - 1 and B are their two sides.  `m > PL_COMPACT_MIN`, the
    # eighth row of kp_init's unrolled loop — full at B, a tail behind it at B + 1 — and every multiple of a tile length,
    # where B + 1 needs one more tile, have a side of their own at B + 1.  The second route level is on from
    # `tiles >= PK_GROUP_MIN`, tiles rounded up: its first chain is (PK_GROUP_MIN - 1) x PK_T + 1 players long.)
    rows = [(WAVE, "wave", False), (geo["KP_INIT_ROW"], "init_row", False), (8 * geo["KP_INIT_ROW"], "init_8rows", True),
            (geo["PL_COMPACT_MIN"], "PL_COMPACT_MIN", True), (geo["PL_MAX"], "PL_MAX", False),
            (geo["NXI_STAGE"], "NXI_STAGE", False),
            ((geo["pair_ptiles"] + 1) * geo["PK_T"], "ptiles+1_x_T", True),
            (geo["PK_TILES_MAX"] * geo["PK_T"], "PK_TILES_MAX_x_T", True),
            ((geo["PK_GROUP_MIN"] - 1) * geo["PK_T"], "PK_GROUP_MIN-1_x_T", True),
            (geo["PK_GROUP_MIN"] * geo["PK_T"], "PK_GROUP_MIN_x_T", True)]
    for i, t in enumerate(T):
        tn = ("T", "T/2", "T/4")[i]
        rows += [(t, tn, True), (2 * t, "2x" + tn, True), (tiles_cap(geo) * t, "cap_x_" + tn, True),
                 (geo["pair_tiles_max"] * t, "tiles_max_x_" + tn, True), (geo["pair_ptiles"] * t, "ptiles_x_" + tn, True)]
    rows += [(s, "seg%d" % s, False) for s in nx_segs(geo)]
    # The 16-bit codes of nx16.  These lengths (and the same distances in pair_distances) CANNOT separate the sides of the
    # encoding: an offset is stored only inside the horizon — two tiles of PK_T, or a chain below PL_MAX — so no stored
    # offset comes near NX_FAR in either geometry, and NX_FAR encoded one lower changes no result of any case.  What
    # the cases do pin is a chain, a stretch of non-fitting players and a partner as long as 2^16 +- 1 positions: index
    # arithmetic that must not pass through 16 bits.  (tests/test_boundaries.py checks NX_FAR < NX_NONE = 0xFFFF, both
    # beyond the longest horizon, from the parsed values.)
    rows += [(geo["NX_FAR"], "NX_FAR", True), (geo["NX_NONE"], "NX_NONE", True), (geo["NX_NONE"] + 1, "2^16", True)]
    return _table(rows, geo)


def team_boundaries(geo):
    """Sorted, de-duplicated chain lengths at which the team path switches: [(B, name, plus, gpu_only)]."""
    rows = [(geo["TT_MIN"], "TT_MIN", False), (geo["TF_BW"] * 32, "TF_BWx32", True),
            (1 << geo["TF_FAR_BITS"], "2^TF_FAR_BITS", True), (geo["TL_BITS_MAX"], "TL_BITS_MAX", True)]
    rows += [(geo["TT_CH"] * k, "TT_CHx%d" % k, True) for k in (1, 2, 8, 9, 32, 33)]
    out = _table(rows, geo)
    # (the team path costs the shim far more per player than the pair path: its longest boundaries stay on the GPU tier
    # only where they are 2^19 or longer — TL_BITS_MAX is not scaled by the small build)
    return [(b, n, plus, b >= (1 << 19)) for b, n, plus, _ in out]


def pair_distances(geo):
    """Distances anchor -> partner (positions of the chain) at which the pair kernels switch: [(X, name, gpu_only)]."""
    T = geo["tile_lengths"]
    rows = [(WAVE, "wave", False), (geo["NXI_STAGE"], "NXI_STAGE", False), (geo["PL_MAX"], "PL_MAX", False)]
    for i, t in enumerate(T):
        tn = ("T", "T/2", "T/4")[i]
        rows += [(t, tn, False), (2 * t, "horizon_" + tn, False)]
    rows += [(s, "seg%d" % s, False) for s in nx_segs(geo)]
    rows += [(geo["NX_FAR"], "NX_FAR", False), (geo["NX_NONE"], "NX_NONE", False), (geo["NX_NONE"] + 1, "2^16", False)]
    return [(b, n, g) for b, n, _, g in _table(rows, geo)]


def lengths(entry):
    """The chain lengths one table entry is tested at."""
    b, _, plus, _ = entry
    return [b - 1, b] + ([b + 1] if plus else [])


# What a tier runs of an entry.  The device runs every entry at every length with both predicates, except the chains of
# 2^19 players and more: one length triple with one predicate each (the oracle walks them on one thread).
# The CPU shim is slow, and its cost grows with the chain and with the passes of the tick: one case with the sparse
# predicate took 3 s at 1536 players, 12 s at 2560, 43 s at 8192 and 73-81 s at 16384 / 16896 (8 cores, -O1 build); with
# the dense predicate 3 s, 4 s, 10 s and 23 s.  The slowest test of the shim tier before these was 35 s.
# So the shim runs the sparse predicate up to PL_MAX only — the longer entries' sparse cases are the device tier's, where the
# same-named entries of the product geometry get both — and, past PK_TILES_MAX tiles of PK_T, B + 1 only where the host
# code branches on `<= B` with a counter to show for it (kp_rounds' reach).
def pair_plan(entry, geo, shim):
    """[(n, predicates)] of one entry of pair_boundaries for one tier."""
    b = entry[0]
    if not shim:
        if b >= 1 << 19:
            return [(n, ("sparse",)) for n in (b - 1, b, b + 1)]
        return [(n, ("sparse", "dense")) for n in lengths(entry)]
    if entry[3]:
        return []
    preds = ("sparse", "dense") if b <= geo["PL_MAX"] else ("dense",)
    ns = lengths(entry)
    if b > geo["PK_TILES_MAX"] * geo["PK_T"] and b != geo["pair_ptiles"] * geo["PK_T"]:
        ns = ns[:2]
    return [(n, preds) for n in ns]


def team_plan(entry, geo, shim):
    """[(n, shapes)] of one entry of team_boundaries for one tier (shapes: "5v5" with cfg-3's role weights, "2v2")."""
    b = entry[0]
    if shim and entry[3]:
        return []
    if b >= 1 << 19:
        return [(n, ("5v5",)) for n in (b - 1, b, b + 1)]
    if shim and b >= 32 * geo["TT_CH"]:
        return [(n, ("5v5",) if n == b else ("2v2",)) for n in lengths(entry)]
    return [(n, ("5v5", "2v2")) for n in lengths(entry)]


def shim_distance_max(geo):
    """The longest distance of pair_distances the shim runs.  The tiny build's horizon is two tiles of 512 positions (or
    a chain below PL_MAX): beyond PL_MAX and four tiles no kernel of that build stores or resolves a distance differently,
    so NXI_STAGE — 8192 in both builds, inside the PRODUCT's horizon of two 8192-tiles only — and the 16-bit distances are
    the device tier's."""
    return max(geo["PL_MAX"], 4 * geo["PK_T"])
