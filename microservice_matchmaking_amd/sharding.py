"""Sharding the search path across the GPUs of one node.

The reference's own partition is the rating group: one queue, one lobby table and one
worker per group, and groups never interact (reference lib/application.ex:26-40,
lib/models/lobby_state.ex:15-29).  Inside a group the stored lobby is selected by
`game_mode` (lib/models/lobby_state.ex:74-83), so two modes of one group never share a lobby
either: the unit that cannot be split is the CHAIN = (game mode, rating group), and the shard
key is exactly that pair.  The path therefore shards with NO data-path collective: every
rank owns one engine and the chains assigned to it, players are routed by
`find_rating_group_by_rating/1` (lib/generic/worker.ex:46-53) and their `"game-mode"`
(lib/search/worker.ex:294) exactly as the Generic worker routes them to per-group AMQP
queues.  torch.distributed (RCCL on GPUs, gloo in the CPU tests) is only used to sum
counters / gather results — and, off the matching path, to carry the players of an mm_move
(include/mm_wait.h) from the rank that owns chain (from_mode, g) to the one that owns chain
(to_mode, g): `ShardedSearch.move` is mm_move_out on every rank, one all-gather of the selected
rows with their stamps, mm_enqueue_stamped on the new owners.  Unlike mm_move on one engine it is
not all-or-nothing: a destination without room raises on every rank after the sources have expired
their players.  `ShardedSearch.rotate` (mm_rotate) is chain-local again: every rank rotates the chains
it owns, no collective; so are `ShardedSearch.locate` (mm_locate) and `ShardedSearch.partners` (mm_partners, in_mode == mode), looks at this rank's own chains.

What this does NOT do, and why: split ONE chain across ranks with a
rating-bucket halo all-gather.  A chain has one open lobby (lobby_state.ex:90-91) and one
cursor; every pass of the cursor depends on the pass before, so a split chain would hop
between devices once per pass (hundreds of passes a tick) — there is no order-free boundary
region to exchange.  A pool of G groups and M modes therefore uses at most G x M ranks, and
the tick of the pool takes as long as its heaviest chain.
"""
from __future__ import annotations

import hashlib

import numpy as np

from ._abi import MMConfig, MMError, NO_SLOT


def rating_groups(cfg: MMConfig, rating) -> np.ndarray:
    """Vectorised find_rating_group_by_rating/1: first inclusive range in table order, else
    the default group (also for NaN = a non-number JSON value)."""
    r = np.asarray(rating, dtype=np.float64)
    out = np.full(r.shape, int(cfg.default_group), dtype=np.uint8)
    done = np.isnan(r)
    for g in range(cfg.n_groups):
        hit = (~done) & (r >= cfg.groups[g].from_) & (r <= cfg.groups[g].to)
        out[hit] = g
        done |= hit
    return out


def chain_weights(cfg: MMConfig, rating, cons) -> np.ndarray:
    """Players per (mode, group) chain of a pool: the load estimate ChainSharding balances."""
    grp = rating_groups(cfg, rating).astype(np.int64)
    mode = (np.asarray(cons, dtype=np.uint32) & 0xF).astype(np.int64)
    ok = mode < cfg.n_modes
    flat = np.bincount(mode[ok] * cfg.n_groups + grp[ok], minlength=cfg.n_modes * cfg.n_groups)
    return flat.reshape(cfg.n_modes, cfg.n_groups).astype(np.float64)


class ChainSharding:
    """(mode, group) -> rank.  Longest-processing-time-first on `weights` (expected load per
    chain, e.g. its share of the pool); equal weights go round robin.  With fewer chains than
    ranks the surplus ranks stay idle (`idle_ranks`) — 7 groups of one mode on 8 GPUs leave
    one GPU without work, by construction of the reference's partition."""

    def __init__(self, n_modes: int, n_groups: int, world_size: int, weights=None):
        self.n_modes, self.n_groups, self.world_size = int(n_modes), int(n_groups), int(world_size)
        if weights is None:
            w = np.ones((self.n_modes, self.n_groups))
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.ndim == 1:                       # one row of group weights for every mode
                w = np.broadcast_to(w, (self.n_modes, self.n_groups)).copy()
        assert w.shape == (self.n_modes, self.n_groups), w.shape
        self.weights = w
        load = np.zeros(self.world_size)
        owner = np.zeros(self.n_modes * self.n_groups, dtype=np.int64)
        for c in np.argsort(-w.ravel(), kind="stable"):
            r = int(np.argmin(load))
            owner[c] = r
            load[r] += max(w.ravel()[c], 1e-12)   # weightless chains still spread out
        self.chain_owner = owner.reshape(self.n_modes, self.n_groups)
        self.load = np.array([w[self.chain_owner == r].sum() for r in range(self.world_size)])

    def chains_of(self, rank: int):
        return [(m, g) for m in range(self.n_modes) for g in range(self.n_groups)
                if self.chain_owner[m, g] == rank]

    def idle_ranks(self):
        used = set(int(r) for r in self.chain_owner.ravel())
        return [r for r in range(self.world_size) if r not in used]

    def bound(self):
        """Total load / heaviest rank.  NOT the speed-up to expect: one GPU already runs all chains concurrently,
        so the pool's step on one GPU is close to its heaviest chain's and sharding gains far less
        (bench.predict_speedup)."""
        top = float(self.load.max())
        return float(self.weights.sum() / top) if top > 0 else 1.0

    def describe(self):
        return {"key": "(game mode, rating group)", "world_size": self.world_size,
                "owner": self.chain_owner.tolist(), "load_share": (self.load / max(self.load.sum(), 1e-12)).tolist(),
                "idle_ranks": self.idle_ranks(), "load_share_bound": self.bound()}


class GroupSharding(ChainSharding):
    """One mode: group -> rank (the round-1 interface, kept for its callers)."""

    def __init__(self, n_groups: int, world_size: int, weights=None):
        super().__init__(1, n_groups, world_size, weights)
        self.owner = self.chain_owner[0]

    def groups_of(self, rank: int):
        return [g for g in range(self.n_groups) if self.owner[g] == rank]


def chain_digest(ids: np.ndarray) -> str:
    """Digest of ONE chain's emission list: the lobbies in publish order, every lobby its
    players' global arrival indices in team order (int64 little endian)."""
    return hashlib.blake2b(np.ascontiguousarray(ids, dtype="<i8").tobytes(), digest_size=16).hexdigest()


def union_digest(per_chain: dict) -> str:
    """Digest of the whole pool's emission: chain digests in (mode, group) order.  A chain that
    emitted nothing contributes the digest of the empty list, so the value does not depend on
    which rank (if any) owned it."""
    h = hashlib.blake2b(digest_size=16)
    for key in sorted(per_chain):
        h.update(("%d/%d:%s;" % (key[0], key[1], per_chain[key])).encode())
    return h.hexdigest()


def tick_digests(mode: int, n_groups: int, ids: np.ndarray, group: np.ndarray) -> dict:
    """{(mode, g): chain_digest} for every group of one tick's match list (ids = global indices)."""
    out = {}
    group = np.asarray(group)
    for g in range(n_groups):
        sel = ids[group == g] if len(ids) else np.zeros((0,), np.int64)
        out[(mode, g)] = chain_digest(sel)
    return out


class ShardedSearch:
    """One rank's share of the search: its engine + the chains it owns."""

    def __init__(self, cfg: MMConfig, engine_cls, rank: int, world_size: int, weights=None):
        self.cfg, self.rank, self.world_size = cfg, rank, world_size
        self.sharding = ChainSharding(cfg.n_modes, cfg.n_groups, world_size, weights)
        self.engine = engine_cls(cfg)
        self.local_to_global = np.full(int(cfg.capacity), -1, dtype=np.int64)   # engine slot -> global arrival index

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def mine(self, rating, cons):
        """Mask of the players of an arrival batch whose chain this rank owns."""
        grp = rating_groups(self.cfg, rating)
        mode = (np.asarray(cons, dtype=np.uint32) & 0xF).astype(np.int64)
        ok = mode < self.cfg.n_modes                      # unknown mode: nobody's (a single engine rejects it)
        own = np.zeros(len(grp), dtype=bool)
        own[ok] = self.sharding.chain_owner[mode[ok], grp[ok].astype(np.int64)] == self.rank
        return own, grp

    def enqueue(self, rating, cons, first_global_index=0):
        """Every rank is handed the same arrival batch (as every Generic worker sees the same
        exchange); it keeps the players whose chain it owns, in arrival order."""
        rating = np.asarray(rating, dtype=np.int32)
        cons = np.asarray(cons, dtype=np.uint32)
        own, grp = self.mine(rating, cons)
        idx = np.nonzero(own)[0]
        slots = self.engine.enqueue(rating[idx], cons[idx], grp[idx])
        ok = slots != NO_SLOT
        self.local_to_global[slots[ok].astype(np.int64)] = first_global_index + idx[ok]
        return idx, slots

    def move(self, from_mode, to_mode, max_age, cons_clear=0):
        """mm_move (include/mm_wait.h).  The moved players keep their global arrival index under their new slot.
        On ONE rank it is the engine's mm_move.  On several, chain (from_mode, g) and chain (to_mode, g) may have different
        owners, and EVERY rank calls this collectively: mm_move_out here, an all-gather of the selected rows (rating group,
        rating, rewritten constraint word, stamp, global index), concatenated in rank order and sorted stably by rating group
        — every chain (from_mode, g) has one owner, so that is the single engine's mm_expired order — and each rank takes the
        rows whose chain (to_mode, group) it owns through mm_enqueue_stamped, stamps and all.
        -> (slots, group, age, new_slots) over the rows THIS rank selected; new_slots is NO_SLOT where the row was refused or
        went to another rank.  self.last_move = {"selected", "taken", "refused"}: this rank's selected rows, the rows it took in
        and the rows it refused as a destination — each sums over the ranks to the one-engine figure.
        Across ranks the move is NOT all-or-nothing: a destination without room raises MMError(MM_ERR_FULL) on every rank,
        after the sources have expired their players and the destinations WITH room have taken theirs in (those players
        wait there under their global index)."""
        if self.world_size != 1:
            return self._move_across_ranks(from_mode, to_mode, lambda: self.engine.move_out(from_mode, to_mode, max_age, cons_clear))
        return self._moved_here(self.engine.move(from_mode, to_mode, max_age, cons_clear))

    def _moved_here(self, got):
        ok = got[3] != NO_SLOT
        self.local_to_global[got[3][ok].astype(np.int64)] = self.local_to_global[got[0][ok].astype(np.int64)]
        return got

    def _chain_local(self, what, mode, rule):
        """The rule's in_mode (None: `mode`), which on several ranks must be `mode`: chain (mode, g) and chain (in_mode, g)
        may have different owners, as for `partners`."""
        in_mode = rule.in_mode if hasattr(rule, "in_mode") else dict(rule).get("in_mode")
        if self.world_size != 1 and in_mode is not None and in_mode != mode:
            raise NotImplementedError("ShardedSearch.%s with in_mode != mode on several ranks: chain (mode %d, g) and chain "
                                      "(in_mode %d, g) may have different owners, and carrying query rows between ranks is "
                                      "not built" % (what, mode, in_mode))

    def move_if(self, from_mode, to_mode, max_age, cons_clear=0, rule=None):
        """mm_move_if (include/mm_wait.h): `move` over the players whose partner count lies in the rule's range.  On ONE
        rank it is the engine's mm_move_if.  On several, with the rule's in_mode == from_mode, the selection is chain-local
        (the candidates are the waiting players of the chain the player sits in, which this rank owns) and the rest is
        `move`'s collective with mm_move_out_if in mm_move_out's place; with in_mode != from_mode the query rows would have
        to travel between ranks: not built, NotImplementedError on every rank."""
        rule = rule or {}
        self._chain_local("move_if", from_mode, rule)
        if self.world_size != 1:
            return self._move_across_ranks(from_mode, to_mode,
                                           lambda: self.engine.move_out_if(from_mode, to_mode, max_age, cons_clear, rule))
        return self._moved_here(self.engine.move_if(from_mode, to_mode, max_age, cons_clear, rule))

    def expire_if(self, mode, max_age, rule):
        """mm_expire_if (include/mm_wait.h).  Chain-local for the rule's in_mode == mode: every rank expires on the chains
        it owns, no collective.  in_mode != mode on several ranks: NotImplementedError on every rank, as `move_if`."""
        self._chain_local("expire_if", mode, rule)
        return self.engine.expire_if(mode, max_age, rule)

    def _move_across_ranks(self, from_mode, to_mode, move_out):
        """`move_out`: this rank's selection call, mm_move_out or mm_move_out_if -> its six columns."""
        if not 0 <= int(to_mode) < self.cfg.n_modes:
            raise MMError(-1, "move across ranks (to_mode)")
        old, group, age, rating, cons, stamp = move_out()
        gid = self.local_to_global[old.astype(np.int64)]
        rows = np.stack([group.astype(np.int64), rating.astype(np.int64), cons.astype(np.int64), stamp.astype(np.int64),
                         gid, np.full(old.size, self.rank, np.int64), np.arange(old.size, dtype=np.int64)], axis=1)
        rows = np.concatenate(self.gather_rows(rows.reshape(-1, 7)))
        rows = rows[np.argsort(rows[:, 0], kind="stable")]
        rows = rows[self.sharding.chain_owner[to_mode, rows[:, 0]] == self.rank]
        new = np.full(old.size, NO_SLOT, dtype=np.uint32)
        status, got = 0, np.zeros(0, np.uint32)
        try:
            if rows.shape[0]:
                got = self.engine.enqueue_stamped(rows[:, 1].astype(np.int32), rows[:, 2].astype(np.uint32),
                                                  rows[:, 3].astype(np.uint32), rows[:, 0].astype(np.uint8))
        except MMError as ex:
            status = ex.status
        ok = got != NO_SLOT
        self.local_to_global[got[ok].astype(np.int64)] = rows[ok, 4]   # (before the raise below: a rank with room has taken its rows)
        # one status for all: a rank that raised alone would leave the others waiting in their next collective
        status = int(-max(self.max_over_ranks([-status])))
        if status:
            raise MMError(status, "move across ranks")
        here = ok & (rows[:, 5] == self.rank)
        new[rows[here, 6]] = got[here]
        self.last_move = {"selected": int(old.size), "taken": int(ok.sum()), "refused": int((~ok).sum())}
        return old, group, age, new

    def rotate(self, mode, max_seated, min_queue=1):
        """mm_rotate (include/mm_wait.h).  Chain-local: a rotated player rejoins the chain it sits in, so every rank rotates
        the chains it owns and no data travels — unlike `move` this is no collective.  The players keep their global arrival
        index under their new slot.  -> (slots, group, age, new_slots) over this rank's chains."""
        got = self.engine.rotate(mode, max_seated, min_queue)
        self.local_to_global[got[3].astype(np.int64)] = self.local_to_global[got[0].astype(np.int64)]
        return got

    def locate(self, mode, slots):
        """mm_locate (include/mm_wait.h).  Chain-local, as `rotate`: `slots` are this rank's engine's slots, the answer is
        about the chains this rank owns, and there is no collective — a status request goes to the rank that holds the
        player.  -> (where, group, position, ahead, age)."""
        return self.engine.locate(mode, slots)

    def partners(self, mode, slots, in_mode=None, window=None, flags=None, by_role=True, gap=True):
        """mm_partners (include/mm_wait.h) for in_mode == mode.  Chain-local, as `locate`: the candidates are the waiting
        players of the chain the queried player sits in, which this rank owns — no collective.  With in_mode != mode the
        chains (mode, g) and (in_mode, g) may have different owners and the query rows would have to travel between ranks:
        not built, NotImplementedError on every rank.  -> (partners, by_role, gap)."""
        if in_mode is not None and in_mode != mode:
            raise NotImplementedError("ShardedSearch.partners with in_mode != mode: chain (mode %d, g) and chain (in_mode %d, g) "
                                      "may have different owners, and carrying query rows between ranks is not built"
                                      % (mode, in_mode))
        return self.engine.partners(mode, slots, None, window, flags, by_role, gap)

    def partner_stats(self, mode, in_mode=None, window=None, flags=None):
        """mm_partner_stats (include/mm_wait.h) for in_mode == mode.  Chain-local, as `partners`: a rank's records are valid
        for the rating groups it owns (the others read as this rank's engine holds them: nobody waiting), and there is no
        collective.  With in_mode != mode the chains (mode, g) and (in_mode, g) may have different owners and the key table
        would have to travel between ranks: not built, NotImplementedError on every rank.  -> one dict per rating group."""
        if in_mode is not None and in_mode != mode:
            raise NotImplementedError("ShardedSearch.partner_stats with in_mode != mode: chain (mode %d, g) and chain (in_mode %d, g) "
                                      "may have different owners, and carrying the sorted table between ranks is not built"
                                      % (mode, in_mode))
        return self.engine.partner_stats(mode, None, window, flags)

    def tick(self, mode=0):
        return self.engine.tick(mode)

    def global_ids(self, matches):
        """Lobbies of a tick with engine slots translated to global arrival indices."""
        if not len(matches):
            return np.zeros(matches.slots.shape, np.int64)
        return self.local_to_global[matches.slots.astype(np.int64)]

    @staticmethod
    def sum_over_ranks(values, op="SUM"):
        """Counters summed over the ranks (the only collective of the matching path)."""
        import torch
        import torch.distributed as dist
        t = torch.tensor([float(v) for v in values], dtype=torch.float64)
        if dist.is_available() and dist.is_initialized():
            if dist.get_backend() == "nccl":
                t = t.cuda()
            dist.all_reduce(t, op=getattr(dist.ReduceOp, op))
        return t.cpu().tolist()

    @staticmethod
    def max_over_ranks(values):
        return ShardedSearch.sum_over_ranks(values, "MAX")

    @staticmethod
    def gather_rows(rows):
        """An (n, c) int64 array of every rank, in rank order (n differs between ranks: the counts go first, the rows
        padded to the longest).  No process group: this rank's alone."""
        import torch
        import torch.distributed as dist
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if not (dist.is_available() and dist.is_initialized()):
            return [rows]
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        world = dist.get_world_size()
        counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([rows.shape[0]], dtype=torch.int64, device=dev))
        counts = [int(c.item()) for c in counts]
        pad = np.zeros((max(counts + [1]), rows.shape[1]), np.int64)
        pad[:rows.shape[0]] = rows
        parts = [torch.zeros(pad.shape, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(pad).to(dev))
        return [p.cpu().numpy()[:k] for p, k in zip(parts, counts)]
