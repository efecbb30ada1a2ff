"""The node: every GPU of one Jylis node behind one C-ABI handle (jy_node_*,
include/jylis_gpu.h, jylis_amd/csrc/jy_node.hip).

One `converge_*` call replaces Database.converge_deltas ->
RepoManagerCore.converge_deltas (jylis/database.pony:50-51,
jylis/repo_manager.pony:92-93) for the whole node: the batch's keys are
hashed on the device, regrouped by owner shard, exchanged (RCCL over xGMI, or
device copies for the single-GPU tests), interned on their owner and merged
there -- all inside the library; the host only reads the per-owner counts
once.  This class is a thin ctypes caller (tests, bench); the Pony host binds
the same entry points.

The converge calls enqueue (round 5): host arrays are copied before a call
returns; device arrays (CUDA tensors) are read later by the node's worker,
so this wrapper keeps them alive until fence() / sync().  The engines
(`engines`, `engine()`) are shared with the worker: use them after sync(),
or inside `with node.locked():`.
"""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import DEVICE, GCOUNT, HOST, PNCOUNT, TLOG, TREG, UJSON
from .engine import Engine, EngineError, _arg, _same_mem, pack_dot, DOT_SEQ_BITS

FABRICS = {"rccl": _lib.FABRIC_RCCL, "copy": _lib.FABRIC_COPY}


def unique_id():
    """a fresh ncclUniqueId (128 bytes) for a multi-process node: made by one
    process, shared with the others (e.g. torch.distributed broadcast)"""
    buf = (C.c_uint8 * 128)()
    rc = _lib.load().jy_node_unique_id(buf)
    if rc != 0:
        raise EngineError(rc, "ncclGetUniqueId failed")
    return bytes(buf)


def _seg_ids(offs):
    offs = np.asarray(offs, np.int64)
    return np.repeat(np.arange(len(offs) - 1), np.diff(offs))


class Node:
    """S key shards, one engine each.  `fabric` "copy": one process, every
    shard local, shards may share a GPU (tests); "rccl": an RCCL
    communicator, one GPU per shard -- all shards local (one process), or
    nlocal = 1 per process with a shared `uid` (unique_id())."""

    def __init__(self, nshards, fabric="copy", devices=None, nlocal=None, rank0=0, uid=None, counter_columns=16,
                 ujson_columns=16, key_capacity=1024, entry_capacity=8192, arena_capacity=1 << 16, flags=0):
        self.lib = _lib.load()
        nlocal = nshards if nlocal is None else nlocal
        if devices is None:
            devices = [0] * nlocal if fabric == "copy" else list(range(rank0, rank0 + nlocal))
        assert len(devices) == nlocal
        cfg = _lib.JyNodeConfig()
        cfg.nshards, cfg.nlocal, cfg.rank0, cfg.fabric = nshards, nlocal, rank0, FABRICS[fabric]
        for i, d in enumerate(devices):
            cfg.devices[i] = d
        if uid is not None:
            assert len(uid) == 128
            for i, b in enumerate(uid):
                cfg.unique_id[i] = b
        self.lib.jy_config_default(C.byref(cfg.engine))
        cfg.engine.counter_columns = counter_columns
        cfg.engine.ujson_columns = ujson_columns
        cfg.engine.flags = flags
        for t in range(5):
            cfg.engine.key_capacity[t] = key_capacity if np.isscalar(key_capacity) else key_capacity[t]
            cfg.engine.entry_capacity[t] = entry_capacity
            cfg.engine.arena_capacity[t] = arena_capacity
        h = C.c_void_p()
        rc = self.lib.jy_node_create(C.byref(cfg), C.byref(h))
        if rc != 0 or not h.value:
            raise EngineError(rc, "jy_node_create failed (no GPU, or RCCL could not form the communicator)")
        self.h = h
        self.S, self.nlocal, self.rank0 = nshards, nlocal, rank0
        self.devices = list(devices)
        self.ujson_columns = ujson_columns
        self.engines = [Engine.attach(self.lib.jy_node_engine(h, rank0 + i), devices[i], ujson_columns)
                        for i in range(nlocal)]
        self._held = []  # device inputs of queued calls (the worker reads them later)
        self._held_mu = threading.Lock()

    def close(self):
        if getattr(self, "h", None):
            for e in self.engines:
                e.close()
            self.lib.jy_node_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.jy_node_last_error(self.h).decode(errors="replace"))

    def sync(self):
        """every queued call done, GPU work included"""
        with self._held_mu:
            held, self._held = self._held, []
        rc = self.lib.jy_node_sync(self.h)  # (drains every stream, failure or not)
        del held
        self._check(rc)

    def fence(self):
        """every queued call issued to the GPU streams (their device inputs are
        then ordered on the node's streams; still alive until the GPU ran)"""
        self._check(self.lib.jy_node_fence(self.h))

    @contextlib.contextmanager
    def locked(self, ctype=None):
        """exclusive use of the node's engines (jy_node_lock / jy_node_unlock);
        with a CRDT type, after that type's queued jobs only
        (jy_node_lock_type; NOFENCE: after none)"""
        rc = self.lib.jy_node_lock(self.h) if ctype is None else self.lib.jy_node_lock_type(self.h, int(ctype))
        try:
            self._check(rc)
            yield self
        finally:
            self.lib.jy_node_unlock(self.h)

    NOFENCE = -1

    def pending(self, ctype=-1):
        """jobs queued or running (of one CRDT type, or all)"""
        n = C.c_uint64()
        self._check(self.lib.jy_node_pending(self.h, int(ctype), C.byref(n)))
        return n.value

    def arena_gc(self, enable=True):
        """the worker reclaims TREG / TLOG arenas after their jobs (jy_node_arena_gc)"""
        self._check(self.lib.jy_node_arena_gc(self.h, 1 if enable else 0))

    def stats(self):
        out = np.zeros(5, np.uint64)
        self._check(self.lib.jy_node_stats(self.h, out.ctypes.data))
        return dict(zip(("keys_in", "keys_received", "bytes_sent", "bytes_received", "exchanges"),
                        (int(x) for x in out)))

    def shard_of(self, key):
        b = key.encode() if isinstance(key, str) else bytes(key)
        buf = C.create_string_buffer(b, len(b) or 1)
        return int(self.lib.jy_node_shard_of(self.h, buf, len(b)))

    def engine(self, shard):
        """the engine of a local shard (reads, local writes, flushes go to the key's owner)"""
        return self.engines[shard - self.rank0]

    def replica_col(self, rid):
        c = C.c_uint32()
        self._check(self.lib.jy_node_replica_col(self.h, C.c_uint64(int(rid) & (2**64 - 1)), C.byref(c)))
        return c.value

    def replica_cols(self, rids):
        return np.array([self.replica_col(r) for r in rids], dtype=np.uint16)

    # -- raw calls (numpy arrays: host; CUDA tensors: device) ----------------
    def _args(self, spec):
        out = [_arg(x, t) for x, t in spec]
        mem = _same_mem(*[m for (k, _, m) in out if k is not None])
        if mem == DEVICE:
            with self._held_mu:
                self._held.append([k for (k, _, _) in out])
        return out, mem

    def counter_converge(self, ctype, kb, ko, cell_offs, col, val, sign=None):
        (k, o, co, c, v, s), mem = self._args([(kb, np.uint8), (ko, np.uint64), (cell_offs, np.uint64),
                                               (col, np.uint16), (val, np.uint64), (sign, np.uint8)])
        n = len(o[0]) - 1
        self._check(self.lib.jy_node_counter_converge(self.h, ctype, n, k[1], o[1], co[1], s[1], c[1], v[1], mem))

    def treg_converge(self, kb, ko, ts, vb, vo):
        (k, o, t, b, bo), mem = self._args([(kb, np.uint8), (ko, np.uint64), (ts, np.uint64), (vb, np.uint8),
                                            (vo, np.uint64)])
        n = len(o[0]) - 1
        self._check(self.lib.jy_node_treg_converge(self.h, n, k[1], o[1], t[1], b[1], bo[1], mem))

    def tlog_converge(self, kb, ko, cutoff, ent_offs, ts, vb, vo):
        (k, o, cu, eo, t, b, bo), mem = self._args([(kb, np.uint8), (ko, np.uint64), (cutoff, np.uint64),
                                                    (ent_offs, np.uint64), (ts, np.uint64), (vb, np.uint8),
                                                    (vo, np.uint64)])
        n = len(o[0]) - 1
        self._check(self.lib.jy_node_tlog_converge(self.h, n, k[1], o[1], cu[1], eo[1], t[1], b[1], bo[1], mem))

    def ujson_converge(self, kb, ko, eo, dots, elems, vvo, vv, co, cloud):
        (k, o, a, d, e, b, v, c, cl), mem = self._args([(kb, np.uint8), (ko, np.uint64), (eo, np.uint64),
                                                        (dots, np.uint64), (elems, np.uint64), (vvo, np.uint64),
                                                        (vv, np.uint64), (co, np.uint64), (cloud, np.uint64)])
        n = len(o[0]) - 1
        self._check(self.lib.jy_node_ujson_converge(self.h, n, k[1], o[1], a[1], d[1], e[1], b[1], v[1], c[1], cl[1],
                                                    mem))

    def counter_converge_block(self, ctype, cols_all, slot0, nslots, vals_p, vals_n=None):
        """dense peer columns arriving mixed: vals_* CUDA tensors [nlocal][ncols][S][nslots];
        cols_all[r][c] = the column of shard r's c-th peer"""
        cols = np.ascontiguousarray(cols_all, np.uint16)
        ncols = cols.shape[1]
        with self._held_mu:
            self._held.append([vals_p, vals_n])
        self._check(self.lib.jy_node_counter_converge_block(
            self.h, ctype, ncols, cols.ctypes.data, slot0, nslots, C.c_void_p(vals_p.data_ptr()),
            None if vals_n is None else C.c_void_p(vals_n.data_ptr())))

    # -- the outbound half: flush_deltas of every local shard, wire form ------
    def flush_wire(self, ctype, device=False, identity=None, leaves=False):
        """flush_deltas() of the node (repo_manager.pony:9): every local shard's
        pending deltas by one wire-form flush each (jy_*_flush_wire), under the
        no-fence lock (a flush reads no state a converge changes; the worker
        may be growing the key directory).  device=True: one wire batch per
        local shard ({name: CUDA tensor}, the arrays the same type's
        converge call takes; complete after sync()) -- nothing crosses the host.
        Otherwise ONE oracle-format batch table, the shards' rows concatenated.
        Counters: `identity` = the writing replica (its column labels the cells).
        leaves=True (UJSON): one wire batch per local shard as well (host arrays
        unless device=True; a batch table has no place for leaves), each with its
        leaf_bytes / leaf_offs, read from the shard's leaf store under the TYPED
        lock (the leaf calls are never made under NOFENCE)."""
        from .repo import concat_tables, wire_to_table
        col = 0
        if ctype in (GCOUNT, PNCOUNT):
            if identity is None:
                raise ValueError("a counter flush needs the writing replica's identity")
            col = self.replica_col(identity)  # (takes the lock itself when the identity is new)
        with_leaves = bool(leaves) and ctype == UJSON
        with self.locked(self.NOFENCE):
            batches = [e.flush_wire(ctype, device, col) for e in self.engines]
            if not with_leaves:
                if device:
                    return batches
                e0 = self.engines[0]
                ids = np.array([e0.replica_id(c) for c in range(e0.replica_count())], np.uint64)
        if with_leaves:
            with self.locked(UJSON):
                return [e.with_leaves(UJSON, b, device) for e, b in zip(self.engines, batches)]
        return concat_tables([wire_to_table(ctype, b, ids) for b in batches])

    def converge_wire(self, ctype, w):
        """one wire batch (flush_wire's arrays, host or device) into this node:
        the same type's converge call, arguments in the batch's order.  A UJSON
        batch that carries leaves has them put into their owner shards' leaf
        stores first (put_leaves)."""
        from .engine import WIRE_ARRAYS, has_leaves
        if ctype == UJSON and has_leaves(w):
            self.put_leaves(w)
        a = [w[name] for name, _, _, _ in WIRE_ARRAYS[ctype]]
        if ctype in (GCOUNT, PNCOUNT):
            kb, ko, co, sign, col, val = a
            self.counter_converge(ctype, kb, ko, co, col, val, sign=sign if ctype == PNCOUNT else None)
        elif ctype == TREG:
            self.treg_converge(*a)
        elif ctype == TLOG:
            self.tlog_converge(*a)
        elif ctype == UJSON:
            self.ujson_converge(*a)
        else:
            raise ValueError(f"unknown CRDT type {ctype}")

    def put_leaves(self, w):
        """the leaves of a UJSON wire batch into the leaf stores of the shards
        that own its documents: each document's owner by jy_keys_owner (the hash
        the node routes by), expanded to a per-element owner through el_offs, then
        one checked put per shard under the typed lock.  The leaf bytes do not
        travel through the node's exchange, so every shard must be local."""
        from .repo import wire_to_host
        from .route import owners
        from .snapshot import permute_items
        if self.nlocal != self.S:
            raise EngineError(_lib.JY_EINVAL, f"a UJSON batch with leaves needs every shard of the node local "
                                              f"({self.nlocal} of {self.S} are): leaves are not routed between processes")
        h = wire_to_host(UJSON, w)
        if len(h["elems"]) == 0:
            return
        own = np.repeat(owners(h["key_bytes"], h["key_offs"], self.S), np.diff(h["el_offs"].astype(np.int64)))
        for s in range(self.S):
            idx = np.nonzero(own == s)[0]
            if len(idx) == 0:
                continue
            lb, lo = permute_items(h["leaf_bytes"], h["leaf_offs"], idx)
            with self.locked(UJSON):
                self.engine(s).put_wire_leaves(h["elems"][idx], lb, lo)

    def ujson_leaves_collect(self, shrink=False):
        """drop the leaves no document refers to from every local shard's leaf
        store (Engine.ujson_leaves_collect) -> the per-shard results, in shard
        order.  Under the typed lock, which waits for the queued UJSON jobs
        whose leaves were already put (put_leaves before converge_wire): every
        such leaf is in a document by the time the mark runs."""
        with self.locked(UJSON):
            return [e.ujson_leaves_collect(shrink=shrink) for e in self.engines]

    # -- state snapshots (jy_*_state_wire): the node's state as wire batches --
    def replica_ids(self):
        """the node's replica id table: ids[c] = the replica id of column c"""
        with self.locked(self.NOFENCE):
            e0 = self.engines[0]
            return [e0.replica_id(c) for c in range(e0.replica_count())]

    def snapshot(self, ctype, max_keys=65536, device=False, leaves=False):
        """the state of one type on every local shard as (shard, wire batch), at
        most max_keys slots per batch, in slot order per shard (a generator).
        Each engine call runs under the TYPED lock (jy_node_lock_type: after the
        type's queued converges -- a snapshot reads state they change, so never
        NOFENCE); the lock is not held between batches, and keys only grow.
        leaves=True: UJSON batches carry their leaves (Engine.with_leaves)."""
        for i, e in enumerate(self.engines):
            with self.locked(ctype):
                n = e.nkeys(ctype)
            for s0 in range(0, n, int(max_keys)):
                with self.locked(ctype):
                    batch = e.state_wire(ctype, s0, min(int(max_keys), n - s0), device, leaves)
                    if device:
                        e.sync()
                yield self.rank0 + i, batch

    # -- keyed reads (jy_*_get_keys): GET of a batch of keys across the shards --
    def get(self, ctype, keys, counts=None):
        """GET of a batch of keys: the query is split by shard_of, each local
        shard answers its keys in ONE keyed read under the typed lock
        (jy_node_lock_type: after the type's queued converges), and the answers
        come back in query order.  Per key: counters the value (0 if missing),
        TREG (value, ts) or None, TLOG [(value, ts)] newest first, at most
        counts[i] of them (counts: None, or one per key, None = every entry)."""
        from .repo import REPOS
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        if ctype not in (GCOUNT, PNCOUNT, TREG, TLOG):
            raise ValueError(f"no keyed read for CRDT type {ctype}")
        if counts is not None and ctype != TLOG:
            raise ValueError("counts apply to TLOG only")
        by_shard = {}
        for i, k in enumerate(keys):
            by_shard.setdefault(self.shard_of(k), []).append(i)
        out = [None] * len(keys)
        for shard, idx in sorted(by_shard.items()):
            e = self.engine(shard)
            mine = [keys[i] for i in idx]
            with self.locked(ctype):
                if ctype in (GCOUNT, PNCOUNT):
                    ans = [int(v) for v in e.counter_get_keys(ctype, mine)[1]]
                elif ctype == TREG:
                    ans = REPOS[TREG](e).get_many(mine)
                else:
                    ans = REPOS[TLOG](e).get_many(mine, None if counts is None else [counts[i] for i in idx])
            for i, a in zip(idx, ans):
                out[i] = a
        return out

    def get_resp(self, ctype, keys, counts=None, what=None, paths=None):
        """GET of a batch of keys answered as RESP reply bytes (jy_*_get_resp):
        the query is split by shard_of, each local shard writes the replies of
        its keys on its GPU in ONE call under the typed lock, and the reply
        spans are put back in query order with one numpy gather -> (bytes,
        offs u64[n + 1]): reply i is bytes[offs[i]:offs[i + 1]].  counts and
        what apply to TLOG only (RepoTLOG.get_resp).  UJSON takes paths (one
        tuple of str per key, None: the whole documents) and returns (bytes,
        offs, on_host u8[n]): where on_host[i] is set the range is empty and
        the caller renders query i (RepoUJSON.get_resp)."""
        from .repo import REPOS
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        if ctype not in (GCOUNT, PNCOUNT, TREG, TLOG, UJSON):
            raise ValueError(f"no keyed read for CRDT type {ctype}")
        if (counts is not None or what is not None) and ctype != TLOG:
            raise ValueError("counts and what apply to TLOG only")
        if paths is not None and ctype != UJSON:
            raise ValueError("paths apply to UJSON only")
        n = len(keys)
        by_shard = {}
        for i, k in enumerate(keys):
            by_shard.setdefault(self.shard_of(k), []).append(i)
        lens = np.zeros(n, np.int64)
        start = np.zeros(n, np.int64)  # where reply i begins in the shards' bytes laid end to end
        on_host = np.zeros(n, np.uint8)
        parts, base = [], 0
        for shard, idx in sorted(by_shard.items()):
            repo = REPOS[ctype](self.engine(shard))
            mine = [keys[i] for i in idx]
            with self.locked(ctype):
                if ctype == TLOG:
                    rb, ro = repo.get_resp(mine, None if counts is None else [counts[i] for i in idx],
                                           None if what is None else [what[i] for i in idx])
                elif ctype == UJSON:
                    rb, ro, oh = repo.get_resp(mine, None if paths is None else [paths[i] for i in idx])
                    on_host[idx] = np.asarray(oh, np.uint8)
                else:
                    rb, ro = repo.get_resp(mine)
            ro = np.asarray(ro, np.uint64).astype(np.int64)
            lens[idx] = np.diff(ro)
            start[idx] = base + ro[:-1]
            parts.append(np.frombuffer(rb, np.uint8))
            base += len(rb)
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        src = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        take = np.repeat(start - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
        if ctype == UJSON:
            return src[take].tobytes(), offs.astype(np.uint64), on_host
        return src[take].tobytes(), offs.astype(np.uint64)

    def write(self, ctype, cmds, identity=None):
        """a batch of write commands, the counterpart of get: the commands are
        split by shard_of, each shard's kept in order, and every local shard
        applies its share in ONE keyed write (jy_*_write_keys / jy_treg_set_keys)
        under the typed lock.  cmds: counters ("INC" | "DEC", key, value) with
        `identity` the writing replica; TREG ("SET", key, value, ts); TLOG as
        RepoTLOG.write takes them."""
        from .repo import REPOS
        if ctype not in (GCOUNT, PNCOUNT, TREG, TLOG):
            raise ValueError(f"no keyed write for CRDT type {ctype}")
        if ctype in (GCOUNT, PNCOUNT) and identity is None:
            raise ValueError("counter writes name the writing replica (identity)")
        known = {GCOUNT: ("INC",), PNCOUNT: ("INC", "DEC"), TREG: ("SET",), TLOG: ("INS", "TRIMAT", "TRIM", "CLR")}
        by_shard = {}
        for c in cmds:
            if c[0] not in known[ctype]:
                raise ValueError(f"{c[0]} is no write command of CRDT type {ctype}")
            k = c[1].encode() if isinstance(c[1], str) else bytes(c[1])
            by_shard.setdefault(self.shard_of(k), []).append((c[0], k) + tuple(c[2:]))
        for shard, mine in sorted(by_shard.items()):
            repo = REPOS[ctype](self.engine(shard))
            with self.locked(ctype):
                if ctype in (GCOUNT, PNCOUNT):
                    # a keyed call per sign; INC and DEC of one key commute (two counters)
                    for sign, name in enumerate(("INC", "DEC")[:1 + (ctype == PNCOUNT)]):
                        sel = [c for c in mine if c[0] == name]
                        if sel:
                            (repo.dec if sign else repo.inc)([c[1] for c in sel], [c[2] for c in sel], identity)
                elif ctype == TREG:
                    repo.set([c[1] for c in mine], [c[2] for c in mine], [c[3] for c in mine])
                else:
                    repo.write(mine)

    # -- state digest and bucket repair (jy_*_state_digest, jy_state_bucket_slots) --
    def digest(self, ctype, nbuckets=1, max_keys=65536):
        """the node's [nbuckets, 4] state digest of one type: the wrapping sum of its
        local shards' digests (the digest is a sum over keys, so it does not depend
        on how many shards hold them).  Each engine call runs under the typed lock."""
        total = np.zeros((int(nbuckets), 4), np.uint64)
        for e in self.engines:
            with self.locked(ctype):
                n = e.nkeys(ctype)
            for s0 in range(0, n, int(max_keys)):
                with self.locked(ctype):
                    d = e.digest_range(ctype, nbuckets, s0, min(int(max_keys), n - s0))
                with np.errstate(over="ignore"):
                    total += d
        return total

    def repair_batches(self, ctype, nbuckets, buckets, max_keys=65536, leaves=False):
        """the state of the keys in `buckets` (of nbuckets key-hash buckets) on every
        local shard as (shard, wire batch), at most max_keys keys per batch: what
        snapshot() yields for all keys, for the buckets a peer's digest differs
        in.  restore() takes them."""
        for i, e in enumerate(self.engines):
            with self.locked(ctype):
                slots = e.bucket_slots(ctype, nbuckets, buckets)
            for a in range(0, len(slots), int(max_keys)):
                with self.locked(ctype):
                    batch = e.state_wire_slots(ctype, slots[a:a + int(max_keys)], leaves=leaves)
                yield self.rank0 + i, batch

    def restore(self, ctype, batches, col_ids=None):
        """converge snapshot batches (wire batches, or snapshot()'s (shard, batch)
        pairs) into this node: one converge_wire each, so every key is re-hashed
        by THIS node's shard count.  col_ids = the source's replica id table
        (replica_ids()): the batches' columns are then rewritten to this node's;
        None: they already are this node's columns."""
        from .repo import wire_to_host
        from .snapshot import remap_columns, sort_dots
        col_map = None if col_ids is None else [self.replica_col(i) for i in col_ids]
        for b in batches:
            if isinstance(b, tuple):
                b = b[1]
            if col_map is not None and col_map != list(range(len(col_map))):
                b = sort_dots(ctype, remap_columns(ctype, wire_to_host(ctype, b), col_map))
            self.converge_wire(ctype, b)

    # -- oracle-format batch tables (the decoded MsgPushDeltas payload) -------
    def converge_table(self, ctype, t):
        """one decoded peer batch in oracle/oracle.py's table layout, as the
        GPU-backed Repo* would marshal it (jylis_amd/repo.py), in ONE node call"""
        kb = np.ascontiguousarray(t["key_bytes"], np.uint8)
        ko = np.ascontiguousarray(t["key_offs"], np.uint64)
        nk = len(ko) - 1
        if ctype == GCOUNT:
            ids = np.asarray(t["ids"], np.uint64)
            cols = self.replica_cols(ids.tolist()) if len(ids) else np.zeros(0, np.uint16)
            self.counter_converge(GCOUNT, kb, ko, np.asarray(t["offs"], np.uint64), cols,
                                  np.asarray(t["vals"], np.uint64))
        elif ctype == PNCOUNT:
            keys, signs, cols, vals = [], [], [], []
            for g, pre in enumerate(("p_", "n_")):
                ids = np.asarray(t[pre + "ids"], np.uint64)
                keys.append(_seg_ids(t[pre + "offs"]))
                signs.append(np.full(len(ids), g, np.uint8))
                cols.append(self.replica_cols(ids.tolist()) if len(ids) else np.zeros(0, np.uint16))
                vals.append(np.asarray(t[pre + "vals"], np.uint64))
            key = np.concatenate(keys)
            order = np.argsort(key, kind="stable")  # every key's cells together
            offs = np.zeros(nk + 1, np.uint64)
            offs[1:] = np.cumsum(np.bincount(key, minlength=nk), dtype=np.uint64)
            self.counter_converge(PNCOUNT, kb, ko, offs, np.concatenate(cols)[order], np.concatenate(vals)[order],
                                  sign=np.concatenate(signs)[order])
        elif ctype == TREG:
            self.treg_converge(kb, ko, np.asarray(t["ts"], np.uint64), np.asarray(t["val_bytes"], np.uint8),
                               np.asarray(t["val_offs"], np.uint64))
        elif ctype == TLOG:
            self.tlog_converge(kb, ko, np.asarray(t["cutoff"], np.uint64), np.asarray(t["ent_offs"], np.uint64),
                               np.asarray(t["ts"], np.uint64), np.asarray(t["val_bytes"], np.uint8),
                               np.asarray(t["val_offs"], np.uint64))
        elif ctype == UJSON:
            self.ujson_converge(*self.ujson_args(t))
        else:
            raise ValueError(f"unknown CRDT type {ctype}")

    def ujson_args(self, t):
        """a UJSON batch table -> the node call's arrays (key bytes, key offsets,
        element offsets, dots, elements, vv offsets, vv, cloud offsets, cloud):
        replica ids to node columns, every document's dots ascending"""
        def packed(ids, seqs, offs, *payload):
            ids = np.asarray(ids, np.uint64)
            seqs = np.asarray(seqs, np.uint64)
            if len(seqs) and (seqs >> np.uint64(DOT_SEQ_BITS)).any():
                raise ValueError("dot sequence numbers must stay below 2^48")
            cols = self.replica_cols(ids.tolist()).astype(np.uint64) if len(ids) else np.zeros(0, np.uint64)
            p = pack_dot(cols, seqs)
            order = np.lexsort((p, _seg_ids(offs)))  # ascending dots per document
            return (p[order],) + tuple(np.asarray(x, np.uint64)[order] for x in payload)
        kb = np.ascontiguousarray(t["key_bytes"], np.uint8)
        ko = np.ascontiguousarray(t["key_offs"], np.uint64)
        eo, vo, co = (np.asarray(t[k], np.uint64) for k in ("el_offs", "vv_offs", "cloud_offs"))
        dots, elems = packed(t["dot_ids"], t["dot_seqs"], eo, t["elems"])
        (vv,) = packed(t["vv_ids"], t["vv_seqs"], vo)
        (cloud,) = packed(t["cloud_ids"], t["cloud_seqs"], co)
        return kb, ko, eo, dots, elems, vo, vv, co, cloud
