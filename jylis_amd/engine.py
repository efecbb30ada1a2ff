"""Python handle over the C ABI of the engine (include/jylis_gpu.h).

Arrays may be numpy (host memory, staged by the engine) or torch CUDA
tensors (HBM-resident, read in stream order).  Each call mirrors one entry
point; higher-level repo semantics live in jylis_amd.repo.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DEVICE, GCOUNT, HOST, PNCOUNT, TLOG, TREG, UJSON

LR_LEN_BITS = 24
LR_LEN_MASK = (1 << LR_LEN_BITS) - 1
DOT_SEQ_BITS = 48
DOT_SEQ_MASK = (1 << DOT_SEQ_BITS) - 1


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"jylis engine error {code}: {msg}")
        self.code = code


# what Engine.ujson_leaves_collect returns (jy_ujson_leaves_collect's out6)
LeavesCollected = collections.namedtuple(
    "LeavesCollected", "kept kept_bytes dropped dropped_bytes elements_without_leaf keep_without_leaf")


def _is_torch(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _arg(x, dtype):
    """-> (keepalive, pointer, mem) for a numpy array or a CUDA tensor."""
    if x is None:
        return None, None, HOST
    if _is_torch(x):
        if not x.is_cuda:
            x = x.numpy()
        else:
            assert x.is_contiguous(), "device arrays must be contiguous"
            assert x.element_size() == np.dtype(dtype).itemsize, (x.dtype, dtype)
            return x, C.c_void_p(x.data_ptr()), DEVICE
    a = np.ascontiguousarray(x, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data), HOST


def _same_mem(*mems):
    ms = {m for m in mems}
    if len(ms) > 1:
        raise ValueError("all arrays of one call must live in the same memory (host or device)")
    return ms.pop() if ms else HOST


def encode_keys(keys):
    """list of str/bytes -> (uint8 bytes, uint64 offsets[n+1])"""
    bs = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    return buf, offs


def pack_dot(col, seq):
    return (np.asarray(col, dtype=np.uint64) << np.uint64(DOT_SEQ_BITS)) | np.asarray(seq, dtype=np.uint64)


def unpack_dot(d):
    d = np.asarray(d, dtype=np.uint64)
    return (d >> np.uint64(DOT_SEQ_BITS)).astype(np.uint32), d & np.uint64(DOT_SEQ_MASK)


TREG_CLAIM_FIELDS = ("pending", "dup_cap", "dup_bound", "seen_words", "unroll", "routed_unroll", "fold_rounds",
                     "tile")


def treg_build_info():
    """the launch geometry libjylis_gpu.so was built with (jy_treg_claim_info of
    no engine: needs no GPU) -> the build's fields of Engine.treg_claim_info"""
    out = np.zeros(8, np.uint64)
    rc = _lib.load().jy_treg_claim_info(None, out.ctypes.data)
    if rc != 0:
        raise EngineError(rc, "jy_treg_claim_info failed")
    return {k: int(v) for k, v in list(zip(TREG_CLAIM_FIELDS, out))[4:]}


class Engine:
    """One engine = one GPU = one key shard."""

    def __init__(self, device=0, counter_columns=16, ujson_columns=16, key_capacity=1024,
                 entry_capacity=8192, arena_capacity=1 << 16, flags=0):
        self.lib = _lib.load()
        cfg = _lib.JyConfig()
        self.lib.jy_config_default(C.byref(cfg))
        cfg.device = device
        cfg.counter_columns = counter_columns
        cfg.ujson_columns = ujson_columns
        cfg.flags = flags
        for t in range(5):
            cfg.key_capacity[t] = key_capacity if np.isscalar(key_capacity) else key_capacity[t]
            cfg.entry_capacity[t] = entry_capacity
            cfg.arena_capacity[t] = arena_capacity
        h = C.c_void_p()
        rc = self.lib.jy_engine_create(C.byref(cfg), C.byref(h))
        if rc != 0 or not h.value:
            raise EngineError(rc, "jy_engine_create failed (no GPU / HIP runtime?)")
        self.h = h
        self.device = device
        self.ujson_columns = ujson_columns

    @classmethod
    def attach(cls, handle, device, ujson_columns=16):
        """a view of an engine someone else owns (a node's shard, jy_node_engine):
        close() leaves it alone"""
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.h = C.c_void_p(handle)
        self.device = device
        self.ujson_columns = ujson_columns
        self._borrowed = True
        return self

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.jy_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.jy_last_error(self.h).decode(errors="replace"))

    def sync(self):
        self._check(self.lib.jy_sync(self.h))

    def set_stream(self, stream_ptr):
        self._check(self.lib.jy_set_stream(self.h, C.c_void_p(stream_ptr)))

    def stream(self):
        return self.lib.jy_get_stream(self.h)

    def timing(self, on=True):
        """bracket every merge call's device work with HIP events (jy_timing_enable)"""
        self._check(self.lib.jy_timing_enable(self.h, 1 if on else 0))

    def timing_read(self, cap=4096):
        """-> per-call device durations (ms) since the last read"""
        out = np.zeros(cap, np.float64)
        n = C.c_uint64()
        self._check(self.lib.jy_timing_read(self.h, cap, out.ctypes.data, C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def skipped(self):
        return int(self.lib.jy_skipped(self.h))

    # -- replicas / keys ---------------------------------------------------
    def replica_col(self, rid):
        c = C.c_uint32()
        self._check(self.lib.jy_replica_col(self.h, C.c_uint64(int(rid) & (2**64 - 1)), C.byref(c)))
        return c.value

    def replica_cols(self, rids):
        return np.array([self.replica_col(r) for r in rids], dtype=np.uint16)

    def replica_id(self, col):
        v = C.c_uint64()
        self._check(self.lib.jy_replica_id(self.h, col, C.byref(v)))
        return v.value

    def replica_count(self):
        return int(self.lib.jy_replica_count(self.h))

    def _keys(self, keys):
        if isinstance(keys, tuple):
            kb, ko = keys
            return np.ascontiguousarray(kb, np.uint8), np.ascontiguousarray(ko, np.uint64)
        return encode_keys(keys)

    def intern(self, ctype, keys):
        kb, ko = self._keys(keys)
        n = len(ko) - 1
        out = np.empty(n, dtype=np.uint32)
        self._check(self.lib.jy_keys_intern(self.h, ctype, n, kb.ctypes.data, ko.ctypes.data, out.ctypes.data))
        return out

    def lookup(self, ctype, keys):
        kb, ko = self._keys(keys)
        n = len(ko) - 1
        out = np.empty(n, dtype=np.uint32)
        self._check(self.lib.jy_keys_lookup(self.h, ctype, n, kb.ctypes.data, ko.ctypes.data, out.ctypes.data))
        return out

    def intern_device(self, ctype, key_bytes, key_offs, create=True):
        """bulk interning with keys already in HBM: key_bytes (uint8) and
        key_offs (int64/uint64, n+1) CUDA tensors -> int32 CUDA tensor of slots"""
        import torch
        n = int(key_offs.numel()) - 1
        out = torch.empty(max(n, 1), dtype=torch.int32, device=key_offs.device)
        fn = self.lib.jy_keys_intern_mem if create else self.lib.jy_keys_lookup_mem
        self._check(fn(self.h, ctype, n, key_bytes.data_ptr(), key_offs.data_ptr(), out.data_ptr(), DEVICE))
        return out[:n]

    def key_names(self, ctype, slot0, n):
        """key strings of slots [slot0, slot0 + n) from the device directory (jy_keys_export)"""
        offs = np.zeros(n + 1, np.uint64)
        if n == 0:
            return []
        self._check(self.lib.jy_keys_export(self.h, ctype, slot0, n, offs.ctypes.data, None, 0))
        buf = np.empty(max(int(offs[-1]), 1), np.uint8)
        self._check(self.lib.jy_keys_export(self.h, ctype, slot0, n, offs.ctypes.data, buf.ctypes.data, len(buf)))
        raw = buf.tobytes()
        return [raw[int(offs[i]):int(offs[i + 1])] for i in range(n)]

    def keys_table(self, ctype):
        """jy_keys_table_read: the device directory as it lies in HBM -> dict of
        tcap, lg, n, blen (ints) and the u64 arrays table[tcap] (tag << 32 |
        slot, ~0 empty), kref[n], khash[n], kw[n, 2]"""
        info = np.zeros(4, np.uint64)
        self._check(self.lib.jy_keys_table_read(self.h, ctype, info.ctypes.data, None, 0, None, None, None, 0))
        tcap, n = int(info[0]), int(info[2])
        table, kref, khash = np.empty(max(tcap, 1), np.uint64), np.empty(max(n, 1), np.uint64), \
            np.empty(max(n, 1), np.uint64)
        kw = np.empty((max(n, 1), 2), np.uint64)
        self._check(self.lib.jy_keys_table_read(self.h, ctype, info.ctypes.data, table.ctypes.data, tcap,
                                                kref.ctypes.data, khash.ctypes.data, kw.ctypes.data, n))
        assert (int(info[0]), int(info[2])) == (tcap, n)
        return {"tcap": tcap, "lg": int(info[1]), "n": n, "blen": int(info[3]), "table": table[:tcap],
                "kref": kref[:n], "khash": khash[:n], "kw": kw[:n]}

    def keys_route_part(self, key_bytes, key_offs, nshards):
        """cross-shard key resolution, sender side (jy_keys_route_part): CUDA
        uint8 key bytes + int64 offsets -> (owner i32[n], pos i32[n], lens
        i64[n], bytes u8, counts i64[2 * nshards]) with the keys in owner order"""
        import torch
        n = int(key_offs.numel()) - 1
        dev = key_offs.device
        own = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        lens = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        byts = torch.empty(max(int(key_bytes.numel()), 1), dtype=torch.uint8, device=dev)
        cnt = torch.empty(2 * nshards, dtype=torch.int64, device=dev)
        self._check(self.lib.jy_keys_route_part(self.h, n, key_bytes.data_ptr(), key_offs.data_ptr(), nshards,
                                                own.data_ptr(), pos.data_ptr(), lens.data_ptr(), byts.data_ptr(),
                                                cnt.data_ptr()))
        return own[:n], pos[:n], lens[:n], byts, cnt

    def keys_intern_lens(self, ctype, key_bytes, lens):
        """intern received keys given as (bytes, lengths) CUDA tensors -> int32 slots (jy_keys_intern_lens)"""
        import torch
        n = int(lens.numel())
        out = torch.empty(max(n, 1), dtype=torch.int32, device=lens.device)
        if n:
            self._check(self.lib.jy_keys_intern_lens(self.h, ctype, n, key_bytes.data_ptr(), lens.data_ptr(),
                                                     out.data_ptr()))
        return out[:n]

    def keys_route_back(self, pos, answers):
        """slots in input order: out[i] = answers[pos[i]] (jy_keys_route_back)"""
        import torch
        n = int(pos.numel())
        out = torch.empty(max(n, 1), dtype=torch.int32, device=pos.device)
        if n:
            self._check(self.lib.jy_keys_route_back(self.h, n, pos.data_ptr(), answers.data_ptr(), out.data_ptr()))
        return out[:n]

    def nkeys(self, ctype):
        return int(self.lib.jy_keys_count(self.h, ctype))

    def reserve(self, ctype, cap):
        self._check(self.lib.jy_keys_reserve(self.h, ctype, cap))

    def pack_values(self, ctype, values):
        """bytes values -> (pre, lr) uint64 arrays; long values go to the arena"""
        vb, vo = encode_keys(values) if not isinstance(values, tuple) else values
        vb = np.ascontiguousarray(vb, np.uint8)
        vo = np.ascontiguousarray(vo, np.uint64)
        n = len(vo) - 1
        pre = np.empty(n, np.uint64)
        lr = np.empty(n, np.uint64)
        self._check(self.lib.jy_values_pack(self.h, ctype, n, vb.ctypes.data, vo.ctypes.data,
                                            pre.ctypes.data, lr.ctypes.data))
        return pre, lr

    # -- keyed writes (k_put.hip): commands by key string, host or device ----
    def _strings(self, x):
        """a list of str/bytes, or (bytes, offs) as numpy arrays or CUDA tensors
        -> (keepalives, bytes pointer, offs pointer, n, mem)"""
        if x is None:
            return None, None, None, None, None
        b, o = x if isinstance(x, tuple) else encode_keys(x)
        kb, pb, mb = _arg(b, np.uint8)
        ko, po, mo = _arg(o, np.uint64)
        if len(kb) == 0:  # no bytes at all: any memory
            mb = mo
        return (kb, ko), pb, po, len(ko) - 1, _same_mem(mb, mo)

    def values_pack_mem(self, ctype, values, device_out=None):
        """jy_values_pack_mem: (pre, lr) handles computed on the device.  values:
        a list of bytes or (bytes, offs) in either memory; the handles come back
        as numpy arrays, or as int64 CUDA tensors with device_out (default: where
        the values live)"""
        keep, pb, po, n, mem = self._strings(values)
        dev = (mem == DEVICE) if device_out is None else device_out
        if dev:
            import torch
            pre = torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{self.device}")
            lr = torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{self.device}")
            ppre, plr = pre.data_ptr(), lr.data_ptr()
        else:
            pre, lr = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
            ppre, plr = pre.ctypes.data, lr.ctypes.data
        self._check(self.lib.jy_values_pack_mem(self.h, ctype, n, pb, po, mem, ppre, plr, DEVICE if dev else HOST))
        del keep
        return pre[:n], lr[:n]

    def counter_write_keys(self, ctype, sign, col, keys, val):
        """jy_counter_write_keys: n INC / DEC of replica column `col` by key
        string (created on a miss); keys may repeat"""
        keep, pkb, pko, n, km = self._strings(keys)
        v, pv, mv = _arg(val if _is_torch(val) else np.asarray(val).astype(np.uint64), np.uint64)
        assert len(v) == n, "one value per key"
        mem = _same_mem(km, mv)
        self._check(self.lib.jy_counter_write_keys(self.h, ctype, sign, col, n, pkb, pko, pv, mem))
        del keep

    def treg_set_keys(self, keys, ts, values):
        """jy_treg_set_keys: n SETs by key string with their value bytes, in order"""
        keep, pkb, pko, n, km = self._strings(keys)
        keepv, pvb, pvo, nv, vm = self._strings(values)
        t, pt, mt = _arg(ts, np.uint64)
        assert nv == n and len(t) == n, "one ts and one value per key"
        mem = _same_mem(km, vm, mt)
        self._check(self.lib.jy_treg_set_keys(self.h, n, pkb, pko, pt, pvb, pvo, mem))
        del keep, keepv

    def tlog_write_keys(self, ops, keys, ts=None, arg=None, values=None):
        """jy_tlog_write_keys: n TLOG commands by key string, applied in order
        however often a key repeats.  A device batch passes every column."""
        keep, pkb, pko, n, km = self._strings(keys)
        keepv, pvb, pvo, nv, vm = self._strings(values)
        o, po, mo = _arg(ops, np.uint8)
        t, pt, mt = _arg(ts, np.uint64)
        a, pa, ma = _arg(arg, np.uint64)
        mems = [km, mo] + [m for x, m in ((ts, mt), (arg, ma), (values, vm)) if x is not None]
        mem = _same_mem(*mems)
        assert len(o) == n and nv in (None, n), "one op (and one value) per key"
        self._check(self.lib.jy_tlog_write_keys(self.h, n, po, pkb, pko, pt, pa, pvb, pvo, mem))
        del keep, keepv

    def tlog_write_rounds(self):
        """jy_tlog_write_rounds: grouped write calls, the last one's rounds, all rounds"""
        out = np.zeros(3, np.uint64)
        self._check(self.lib.jy_tlog_write_rounds(self.h, out.ctypes.data))
        return dict(zip(("calls", "last", "total"), (int(x) for x in out)))

    def ujson_write_keys(self, ops, keys, leaves, identity):
        """jy_ujson_write_keys: n UJSON INS / RM / CLR commands by key string,
        applied in order to replica `identity`'s column however often a key
        repeats.  ops: UJSON_INS / _RM / _CLR; leaves: a list of leaf encodings
        (ujson_doc._encode; b"" for a CLR) or (bytes, offs), in the memory of
        the keys.  INS creates its key and puts its leaf into the leaf store; RM
        / CLR of a missing key do nothing.  The caller holds the leaf store's lock."""
        keep, pkb, pko, n, km = self._strings(keys)
        keepl, plb, plo, nl, lm = self._strings(leaves)
        o, po, mo = _arg(ops, np.uint8)
        assert len(o) == n and nl == n, "one op and one leaf per key"
        mem = _same_mem(km, mo, lm)
        self._check(self.lib.jy_ujson_write_keys(self.h, n, po, pkb, pko, plb, plo, int(identity), mem))
        del keep, keepl

    UJSON_WRITE_KEYS_INFO = ("calls", "rounds_last", "rounds_total", "applied", "skipped", "leaves_put")

    def ujson_write_keys_info(self):
        """jy_ujson_write_keys_info: calls that applied their batch, the last
        one's rounds, all rounds, and the last call's commands applied, RM / CLR
        skipped for a missing key, INS leaves handed to the leaf store"""
        out = np.zeros(6, np.uint64)
        self._check(self.lib.jy_ujson_write_keys_info(self.h, out.ctypes.data))
        return dict(zip(self.UJSON_WRITE_KEYS_INFO, (int(x) for x in out)))

    def arena_usage(self, ctype):
        n, c = C.c_uint64(), C.c_uint64()
        self._check(self.lib.jy_arena_usage(self.h, ctype, C.byref(n), C.byref(c)))
        return n.value, c.value

    def arena_reserve(self, ctype, nbytes):
        """room for `nbytes` at the tail of a type's value arena (jy_arena_reserve):
        (device pointer, arena offset); valid until the arena next grows"""
        p, r = C.c_void_p(), C.c_uint64()
        self._check(self.lib.jy_arena_reserve(self.h, ctype, nbytes, C.byref(p), C.byref(r)))
        return p.value or 0, r.value

    def arena_collect(self, ctype):
        """reclaim dead value bytes (jy_arena_collect); unmerged packed handles become invalid.
        Refused while a router holds rounds of this engine's batches in flight: their
        handles would be read again by a drain round (route.py _RunRouter)."""
        holds = getattr(self, "_route_holds", None)
        if holds:
            raise RuntimeError("arena_collect while a router has rounds in flight on this engine: "
                               "call router.drain() first")
        live = C.c_uint64()
        self._check(self.lib.jy_arena_collect(self.h, ctype, C.byref(live)))
        return live.value

    def arena_read(self, ctype, off, n):
        buf = np.empty(max(n, 1), np.uint8)
        self._check(self.lib.jy_arena_read(self.h, ctype, off, n, buf.ctypes.data))
        return bytes(buf[:n])

    def value_bytes(self, ctype, pre, lr):
        """(pre, lr) handle -> bytes"""
        pre, lr = int(pre), int(lr)
        n = lr & LR_LEN_MASK
        if n <= 8:
            return pre.to_bytes(8, "big")[:n]
        return self.arena_read(ctype, lr >> LR_LEN_BITS, n)

    # -- GCOUNT / PNCOUNT --------------------------------------------------
    def gcount_converge(self, slot, col, val):
        a, pa, ma = _arg(slot, np.uint32)
        b, pb, mb = _arg(col, np.uint16)
        c, pc, mc = _arg(val, np.uint64)
        mem = _same_mem(ma, mb, mc)
        self._check(self.lib.jy_gcount_converge(self.h, len(a), pa, pb, pc, mem))

    def counter_converge_keys(self, ctype, keys, col, val, cell_key=None, sign=None):
        """one peer batch with its key strings (jy_counter_converge_keys):
        keys interned on the device, cells merged with the device slots.
        Host keys (list or (bytes, offs)) with host cells, or CUDA tensors
        throughout (keys as (uint8 bytes, int64 offs))."""
        if isinstance(keys, tuple) and hasattr(keys[0], "data_ptr"):
            kb, ko = keys
            nk = int(ko.numel()) - 1
            pkb, pko = C.c_void_p(kb.data_ptr()), C.c_void_p(ko.data_ptr())
            km = DEVICE
        else:
            kb, ko = self._keys(keys)
            nk = len(ko) - 1
            pkb, pko = kb.ctypes.data, ko.ctypes.data
            km = HOST
        c, pc, mc = _arg(col, np.uint16)
        v, pv, mv = _arg(val, np.uint64)
        args = [(c, mc), (v, mv)]
        pk = ps = None
        if cell_key is not None:
            k_, pk, mk = _arg(cell_key, np.uint32)
            args.append((k_, mk))
        if sign is not None:
            s_, ps, ms = _arg(sign, np.uint8)
            args.append((s_, ms))
        mem = _same_mem(km, *[m for _, m in args])
        self._check(self.lib.jy_counter_converge_keys(self.h, ctype, nk, pkb, pko, len(c), pk, ps, pc, pv, mem))

    def gcount_converge_block(self, cols, slot0, vals):
        cols = np.ascontiguousarray(cols, np.uint16)
        v, pv, mv = _arg(vals, np.uint64)
        ncols = len(cols)
        nslots = (v.shape[-1] if v.ndim > 1 else (len(v) // max(ncols, 1)))
        self._check(self.lib.jy_gcount_converge_block(self.h, ncols, cols.ctypes.data, slot0, nslots, pv, mv))

    def gcount_get(self, slots):
        s, ps, ms = _arg(slots, np.uint32)
        if ms == DEVICE:
            import torch
            out = torch.empty(len(s), dtype=torch.int64, device=s.device)
            self._check(self.lib.jy_gcount_get(self.h, len(s), ps, C.c_void_p(out.data_ptr()), DEVICE))
            return out
        out = np.empty(len(s), np.uint64)
        self._check(self.lib.jy_gcount_get(self.h, len(s), ps, out.ctypes.data, HOST))
        return out

    def pncount_converge(self, p=None, n=None):
        """p / n: (slot, col, val) triples (either may be None)"""
        ps = [_arg(x, t) for x, t in zip(p or (None, None, None), (np.uint32, np.uint16, np.uint64))]
        ns = [_arg(x, t) for x, t in zip(n or (None, None, None), (np.uint32, np.uint16, np.uint64))]
        mems = [m for (k, _, m) in ps + ns if k is not None]
        mem = _same_mem(*mems)
        np_ = len(ps[0][0]) if ps[0][0] is not None else 0
        nn = len(ns[0][0]) if ns[0][0] is not None else 0
        self._check(self.lib.jy_pncount_converge(self.h, np_, ps[0][1], ps[1][1], ps[2][1],
                                                 nn, ns[0][1], ns[1][1], ns[2][1], mem))

    def pncount_converge_block(self, cols, slot0, vals_p, vals_n):
        cols = np.ascontiguousarray(cols, np.uint16)
        a, pa, ma = _arg(vals_p, np.uint64)
        b, pb, mb = _arg(vals_n, np.uint64)
        mem = _same_mem(ma, mb)
        ncols = len(cols)
        nslots = a.shape[-1] if a.ndim > 1 else len(a) // max(ncols, 1)
        self._check(self.lib.jy_pncount_converge_block(self.h, ncols, cols.ctypes.data, slot0, nslots, pa, pb, mem))

    def pncount_get(self, slots):
        s, ps, ms = _arg(slots, np.uint32)
        if ms == DEVICE:
            import torch
            out = torch.empty(len(s), dtype=torch.int64, device=s.device)
            self._check(self.lib.jy_pncount_get(self.h, len(s), ps, C.c_void_p(out.data_ptr()), DEVICE))
            return out
        out = np.empty(len(s), np.int64)
        self._check(self.lib.jy_pncount_get(self.h, len(s), ps, out.ctypes.data, HOST))
        return out

    def counter_export(self, ctype, ncols, slot0, nslots):
        nsigns = 1 if ctype == GCOUNT else 2
        out = np.zeros((nsigns, ncols, nslots), np.uint64)
        self._check(self.lib.jy_counter_export(self.h, ctype, ncols, slot0, nslots, out.ctypes.data))
        return out

    # -- counter write path (RepoGCOUNT.inc / RepoPNCOUNT.inc,dec) + flush --
    def counter_write(self, ctype, sign, col, slot, val):
        """n local writes under replica column `col`: s[slot][col] += val
        (wrapping); sign 0 = INC, 1 = DEC (PNCOUNT).  val: uint64 (an i64
        argument bit-cast, repo_pncount.pony:60,65)"""
        a, pa, ma = _arg(slot, np.uint32)
        b, pb, mb = _arg(val if _is_torch(val) else np.asarray(val).astype(np.uint64), np.uint64)
        mem = _same_mem(ma, mb)
        self._check(self.lib.jy_counter_write(self.h, ctype, sign, col, len(a), pa, pb, mem))

    def counter_deltas_size(self, ctype):
        n = C.c_uint64()
        self._check(self.lib.jy_counter_deltas_size(self.h, ctype, C.byref(n)))
        return n.value

    def counter_flush(self, ctype):
        """flush_deltas -> (slots u32[n], vals u64[nsigns][n], mask u32[n])"""
        nsigns = 1 if ctype == GCOUNT else 2
        cap = self.counter_deltas_size(ctype)
        slots = np.zeros(max(cap, 1), np.uint32)
        vals = np.zeros((nsigns, max(cap, 1)), np.uint64)
        mask = np.zeros(max(cap, 1), np.uint32)
        n = C.c_uint64()
        self._check(self.lib.jy_counter_flush(self.h, ctype, max(cap, 1), slots.ctypes.data, vals.ctypes.data,
                                              mask.ctypes.data, C.byref(n), HOST))
        k = n.value
        return slots[:k].copy(), vals[:, :k].copy(), mask[:k].copy()

    # -- TREG --------------------------------------------------------------
    def treg_converge(self, slot, ts, pre, lr):
        a, pa, ma = _arg(slot, np.uint32)
        b, pb, mb = _arg(ts, np.uint64)
        c, pc, mc = _arg(pre, np.uint64)
        d, pd, md = _arg(lr, np.uint64)
        mem = _same_mem(ma, mb, mc, md)
        self._check(self.lib.jy_treg_converge(self.h, len(a), pa, pb, pc, pd, mem))

    def treg_converge_block(self, slot0, ts, pre, lr):
        """a block batch (jy_treg_converge_block): entry i is slot slot0 + i"""
        b, pb, mb = _arg(ts, np.uint64)
        c, pc, mc = _arg(pre, np.uint64)
        d, pd, md = _arg(lr, np.uint64)
        mem = _same_mem(mb, mc, md)
        self._check(self.lib.jy_treg_converge_block(self.h, int(slot0), len(b), pb, pc, pd, mem))

    def treg_set(self, slot, ts, pre, lr):
        """local SETs (RepoTREG.set): state LWW + pending delta"""
        a, pa, ma = _arg(slot, np.uint32)
        b, pb, mb = _arg(ts, np.uint64)
        c, pc, mc = _arg(pre, np.uint64)
        d, pd, md = _arg(lr, np.uint64)
        mem = _same_mem(ma, mb, mc, md)
        self._check(self.lib.jy_treg_set(self.h, len(a), pa, pb, pc, pd, mem))

    def treg_deltas_size(self):
        n = C.c_uint64()
        self._check(self.lib.jy_treg_deltas_size(self.h, C.byref(n)))
        return n.value

    def treg_flush(self):
        """flush_deltas -> (slots, ts, pre, lr) of every pending key"""
        cap = max(self.treg_deltas_size(), 1)
        slots = np.zeros(cap, np.uint32)
        ts, pre, lr = (np.zeros(cap, np.uint64) for _ in range(3))
        n = C.c_uint64()
        self._check(self.lib.jy_treg_flush(self.h, cap, slots.ctypes.data, ts.ctypes.data, pre.ctypes.data,
                                           lr.ctypes.data, C.byref(n), HOST))
        k = n.value
        return slots[:k].copy(), ts[:k].copy(), pre[:k].copy(), lr[:k].copy()

    def treg_read(self, slots):
        s = np.ascontiguousarray(slots, np.uint32)
        n = len(s)
        ts, pre, lr = (np.empty(n, np.uint64) for _ in range(3))
        self._check(self.lib.jy_treg_read(self.h, n, s.ctypes.data, ts.ctypes.data, pre.ctypes.data, lr.ctypes.data))
        return ts, pre, lr

    def treg_claim_info(self):
        """jy_treg_claim_info: the merges' first-occurrence claim, read without
        folding -> {"pending", "dup_cap", "dup_bound", "seen_words", "unroll",
        "routed_unroll", "fold_rounds", "tile": int} (pending: records in the
        duplicate list, as the device counts them)"""
        out = np.zeros(8, np.uint64)
        self._check(self.lib.jy_treg_claim_info(self.h, out.ctypes.data))
        return dict(zip(TREG_CLAIM_FIELDS, (int(x) for x in out)))

    # -- TLOG --------------------------------------------------------------
    def tlog_converge(self, slot, cutoff, ent_offs, ts, pre, lr):
        a, pa, ma = _arg(slot, np.uint32)
        b, pb, mb = _arg(cutoff, np.uint64)
        c, pc, mc = _arg(ent_offs, np.uint64)
        d, pd, md = _arg(ts, np.uint64)
        e, pe, me = _arg(pre, np.uint64)
        f, pf, mf = _arg(lr, np.uint64)
        mem = _same_mem(ma, mb, mc, md, me, mf)
        self._check(self.lib.jy_tlog_converge(self.h, len(a), pa, pb, pc, len(d), pd, pe, pf, mem))

    def tlog_write(self, ops, slot, ts=None, arg=None, pre=None, lr=None):
        """RepoTLOG.ins / trimat / trim / clr commands (jy_tlog_write), in order"""
        n = len(slot)
        cols = []
        for x, t in ((ops, np.uint8), (slot, np.uint32), (ts, np.uint64), (arg, np.uint64), (pre, np.uint64),
                     (lr, np.uint64)):
            cols.append(_arg(np.zeros(n, t) if x is None else x, t))
        mem = _same_mem(*[m for (_, _, m) in cols])
        (o, po, _), (s, ps, _), (a, pa, _), (b, pb, _), (c, pc, _), (d, pd, _) = cols
        self._check(self.lib.jy_tlog_write(self.h, n, po, ps, pa, pb, pc, pd, mem))

    def tlog_deltas_size(self):
        n = C.c_uint64()
        self._check(self.lib.jy_tlog_deltas_size(self.h, C.byref(n)))
        return n.value

    def tlog_flush(self):
        """flush_deltas -> (slots, cutoffs, offs, ts, pre, lr) of every pending key"""
        k, m = C.c_uint64(), C.c_uint64()
        z = np.zeros(1, np.uint64)
        self._check(self.lib.jy_tlog_flush(self.h, 0, 0, None, None, None, None, None, None, C.byref(k), C.byref(m),
                                           HOST))
        nk, ne = k.value, m.value
        slots = np.zeros(max(nk, 1), np.uint32)
        cut = np.zeros(max(nk, 1), np.uint64)
        offs = np.zeros(nk + 1, np.uint64)
        ts, pre, lr = (np.zeros(max(ne, 1), np.uint64) for _ in range(3))
        if nk:
            self._check(self.lib.jy_tlog_flush(self.h, nk, ne, slots.ctypes.data, cut.ctypes.data, offs.ctypes.data,
                                               ts.ctypes.data, pre.ctypes.data, lr.ctypes.data, C.byref(k),
                                               C.byref(m), HOST))
        del z
        return slots[:nk].copy(), cut[:nk].copy(), offs, ts[:ne].copy(), pre[:ne].copy(), lr[:ne].copy()

    def tlog_stats(self):
        """jy_tlog_stats: merges issued, spilled (re-merged after a compaction), compactions, pool capacity"""
        out = np.zeros(4, np.uint64)
        self._check(self.lib.jy_tlog_stats(self.h, out.ctypes.data))
        return dict(zip(("merges", "spills", "compactions", "pool_entries"), (int(x) for x in out)))

    def tlog_layout(self, slots):
        """jy_tlog_layout: where the state store keeps the logs of host slots ->
        {"base", "front", "len", "cap", "cutoff", "newest": u64[n], "pcap", "used": int}
        (used: the pool's bump pointer)"""
        s = np.ascontiguousarray(slots, np.uint32)
        n = len(s)
        out = np.zeros(6 * n + 2, np.uint64)
        self._check(self.lib.jy_tlog_layout(self.h, n, s.ctypes.data, out.ctypes.data))
        lay = {name: out[i * n:(i + 1) * n].copy()
               for i, name in enumerate(("base", "front", "len", "cap", "cutoff", "newest"))}
        lay["pcap"], lay["used"] = int(out[6 * n]), int(out[6 * n + 1])
        return lay

    def tlog_read(self, slots):
        """-> (cutoff[n], offs[n+1], ts, pre, lr) for host slots"""
        s = np.ascontiguousarray(slots, np.uint32)
        n = len(s)
        lens = np.empty(n, np.uint64)
        cut = np.empty(n, np.uint64)
        self._check(self.lib.jy_tlog_read_sizes(self.h, n, s.ctypes.data, lens.ctypes.data, cut.ctypes.data))
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        m = int(offs[-1])
        ts, pre, lr = (np.empty(max(m, 1), np.uint64) for _ in range(3))
        self._check(self.lib.jy_tlog_read(self.h, n, s.ctypes.data, offs.ctypes.data, ts.ctypes.data,
                                          pre.ctypes.data, lr.ctypes.data))
        return cut, offs, ts[:m], pre[:m], lr[:m]

    # -- UJSON -------------------------------------------------------------
    def ujson_converge(self, slot, el_offs, dots, elems, vv_offs, vv, cloud_offs, cloud):
        args = [_arg(x, t) for x, t in ((slot, np.uint32), (el_offs, np.uint64), (dots, np.uint64),
                                        (elems, np.uint64), (vv_offs, np.uint64), (vv, np.uint64),
                                        (cloud_offs, np.uint64), (cloud, np.uint64))]
        mem = _same_mem(*[m for (_, _, m) in args])
        (s, ps, _), (eo, peo, _), (d, pd, _), (e, pe, _), (vo, pvo, _), (v, pv, _), (co, pco, _), (c, pc, _) = args
        self._check(self.lib.jy_ujson_converge(self.h, len(s), ps, peo, len(d), pd, pe, pvo, len(v), pv,
                                               pco, len(c), pc, mem))

    def ujson_write(self, ops, slot, elem, col):
        """RepoUJSON.ins / rm / clr on opaque element handles (jy_ujson_write), in order"""
        n = len(slot)
        o, po, mo = _arg(ops, np.uint8)
        s, ps, ms = _arg(slot, np.uint32)
        e, pe, me = _arg(np.zeros(n, np.uint64) if elem is None else elem, np.uint64)
        self._check(self.lib.jy_ujson_write(self.h, n, po, ps, pe, int(col), _same_mem(mo, ms, me)))

    def ujson_deltas_size(self):
        n = C.c_uint64()
        self._check(self.lib.jy_ujson_deltas_size(self.h, C.byref(n)))
        return n.value

    def ujson_flush(self):
        """flush_deltas -> (slots, el_offs, dots, elems, vv[n][R], cloud_offs, cloud) of every pending doc"""
        k, me, mc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.jy_ujson_flush(self.h, 0, 0, 0, None, None, None, None, None, None, None,
                                            C.byref(k), C.byref(me), C.byref(mc), HOST))
        nk, ne, nc = k.value, me.value, mc.value
        R = self.ujson_columns
        slots = np.zeros(max(nk, 1), np.uint32)
        eo = np.zeros(nk + 1, np.uint64)
        co = np.zeros(nk + 1, np.uint64)
        dots, elems = np.zeros(max(ne, 1), np.uint64), np.zeros(max(ne, 1), np.uint64)
        cloud = np.zeros(max(nc, 1), np.uint64)
        vv = np.zeros((max(nk, 1), R), np.uint64)
        if nk:
            self._check(self.lib.jy_ujson_flush(self.h, nk, ne, nc, slots.ctypes.data, eo.ctypes.data,
                                                dots.ctypes.data, elems.ctypes.data, vv.ctypes.data, co.ctypes.data,
                                                cloud.ctypes.data, C.byref(k), C.byref(me), C.byref(mc), HOST))
        return slots[:nk].copy(), eo, dots[:ne].copy(), elems[:ne].copy(), vv[:nk].copy(), co, cloud[:nc].copy()

    UJSON_STATS = ("touched_el", "touched_cloud", "out_el", "out_cloud", "delta_el", "delta_cloud", "delta_docs",
                   "calls", "inplace_docs", "inplace_state_el", "inplace_state_cloud", "inplace_added_el",
                   "inplace_added_cloud", "inplace_folded", "promoted", "demoted")

    def ujson_stats(self):
        """cumulative converge counters (jy_ujson_stats_ext): dict of touched /
        written / delta sizes of the regular merge path, then the in-place
        layout's documents, their untouched state sizes, what they appended
        and folded, promotions and demotions"""
        out = np.zeros(16, np.uint64)
        self._check(self.lib.jy_ujson_stats_ext(self.h, out.ctypes.data))
        return {k: int(v) for k, v in zip(self.UJSON_STATS, out)}

    def ujson_set_inplace(self, min_elems):
        """promotion threshold of the UJSON in-place layout (0: no promotions)"""
        self._check(self.lib.jy_ujson_set_inplace(self.h, int(min_elems)))

    def ujson_read(self, slots):
        """-> (el_offs, dots, elems, vv[n][R], cloud_offs, cloud)"""
        s = np.ascontiguousarray(slots, np.uint32)
        n = len(s)
        nel = np.empty(n, np.uint64)
        ncl = np.empty(n, np.uint64)
        self._check(self.lib.jy_ujson_read_sizes(self.h, n, s.ctypes.data, nel.ctypes.data, ncl.ctypes.data))
        eo = np.zeros(n + 1, np.uint64)
        eo[1:] = np.cumsum(nel, dtype=np.uint64)
        co = np.zeros(n + 1, np.uint64)
        co[1:] = np.cumsum(ncl, dtype=np.uint64)
        me, mc = int(eo[-1]), int(co[-1])
        dots = np.empty(max(me, 1), np.uint64)
        elems = np.empty(max(me, 1), np.uint64)
        vv = np.empty((max(n, 1), self.ujson_columns), np.uint64)
        cloud = np.empty(max(mc, 1), np.uint64)
        self._check(self.lib.jy_ujson_read(self.h, n, s.ctypes.data, eo.ctypes.data, dots.ctypes.data,
                                           elems.ctypes.data, vv.ctypes.data, co.ctypes.data, cloud.ctypes.data))
        return eo, dots[:me], elems[:me], vv[:n], co, cloud[:mc]


    # -- wire-form flush (jy_*_flush_wire): flush_deltas as a converge batch --
    def flush_wire_caps(self, ctype, caps, device=False, col=0):
        """one jy_*_flush_wire call with the given output capacities (WIRE_SIZES[ctype]
        order) -> (sizes needed, {name: array}).  The arrays (numpy, or CUDA tensors
        with device=True; WIRE_ARRAYS[ctype] order) hold exactly `caps` elements,
        offsets one more; they are filled, and the pending set cleared, only when no
        capacity is short.  Device outputs are uninitialised until then (the engine
        writes them on its own stream) and complete after sync()."""
        head = [ctype, int(col)] if ctype in (GCOUNT, PNCOUNT) else []
        return self._wire_call(_WIRE_FN[ctype], ctype, head, caps, True, device)

    def _wire_call(self, fn, ctype, head, caps, keys_cap, device, out=None):
        """one engine call that writes a wire batch: the WIRE_ARRAYS[ctype] outputs
        for the capacities `caps` (made here: numpy, or CUDA tensors with device=True;
        or the caller's `out`, checked to be large enough), then fn(engine, *head,
        *caps, *arrays, sizes, mem) -> (sizes needed, {name: array}).  keys_cap:
        the call takes caps[0] (the snapshots do not: their per-key arrays hold
        caps[0] elements by contract)."""
        caps = [int(c) for c in caps]
        assert len(caps) == len(WIRE_SIZES[ctype])
        arrays, ptrs = {}, []
        for name, dt, idx, plus in WIRE_ARRAYS[ctype]:
            n = caps[idx] + plus
            if out is not None:
                a = out[name]
                assert len(a) >= n, name
            elif device:
                import torch
                a = torch.empty(max(n, 1), dtype=getattr(torch, TORCH_DTYPE[dt]), device=f"cuda:{self.device}")
            else:
                a = np.zeros(max(n, 1), dt)
            ptrs.append(C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data))
            arrays[name] = a[:n]
        sizes = (C.c_uint64 * len(caps))()
        self._check(getattr(self.lib, fn)(self.h, *head, *caps[0 if keys_cap else 1:], *ptrs, sizes,
                                          DEVICE if device else HOST))
        return [int(x) for x in sizes], arrays

    def _wire_two_phase(self, ctype, call, device, leaves):
        """call(caps) -> (sizes, arrays) made twice: one call sizes the batch, one
        fills it -> the batch, each array cut to its size"""
        need, _ = call([0] * len(WIRE_SIZES[ctype]))
        sizes, out = call(need)
        assert sizes == need, (sizes, need)
        w = {name: out[name][:sizes[idx] + plus] for name, _, idx, plus in WIRE_ARRAYS[ctype]}
        return self.with_leaves(ctype, w, device) if leaves else w

    def flush_wire(self, ctype, device=False, col=0, leaves=False):
        """flush_deltas() of one type as the arrays its jy_node_*_converge takes
        ({name: array} in argument order; counters: `col` = the writing replica's
        column).  The first call is made with the capacities the previous flush of
        this type needed, so a steady heartbeat flushes in ONE engine call; only a
        batch that outgrew them costs a second call with the sizes the first reported.
        leaves=True (UJSON): the batch also carries leaf_bytes / leaf_offs, the
        encoded leaf of every element (with_leaves)."""
        memo = self.__dict__.setdefault("_wire_caps", {})
        key = (ctype, bool(device))
        sizes, out = self.flush_wire_caps(ctype, memo.get(key, [0] * len(WIRE_SIZES[ctype])), device, col)
        if any(s > c for s, c in zip(sizes, memo.get(key, [0] * len(sizes)))):
            need = sizes
            sizes, out = self.flush_wire_caps(ctype, need, device, col)
            assert sizes == need, (sizes, need)
        if sizes[0]:
            memo[key] = sizes
        w = {name: out[name][:sizes[idx] + plus] for name, _, idx, plus in WIRE_ARRAYS[ctype]}
        return self.with_leaves(ctype, w, device) if leaves else w

    def counter_flush_wire(self, ctype, col, device=False):
        return self.flush_wire(ctype, device, col)

    def treg_flush_wire(self, device=False):
        return self.flush_wire(TREG, device)

    def tlog_flush_wire(self, device=False):
        return self.flush_wire(TLOG, device)

    def ujson_flush_wire(self, device=False, leaves=False):
        return self.flush_wire(UJSON, device, leaves=leaves)

    # -- UJSON leaf store (jy_ujson_leaves_*): the leaves behind the element handles --
    def ujson_leaves_put(self, leaf_bytes, leaf_offs):
        """store n encoded leaves (packed bytes, offsets[n + 1]; numpy, or CUDA
        tensors) -> their handles (numpy uint64, or an int64 CUDA tensor complete
        after sync()); 0 for a malformed item or a 64-bit collision"""
        b, pb, mb = _arg(leaf_bytes, np.uint8)
        o, po, mo = _arg(leaf_offs, np.uint64)
        mem = _same_mem(mb, mo)
        n = len(o) - 1
        if mem == DEVICE:
            import torch
            out = torch.empty(max(n, 1), dtype=torch.int64, device=f"cuda:{self.device}")
            ptr = C.c_void_p(out.data_ptr())
        else:
            out = np.zeros(max(n, 1), np.uint64)
            ptr = C.c_void_p(out.ctypes.data)
        self._check(self.lib.jy_ujson_leaves_put(self.h, n, pb, po, ptr, mem))
        return out[:n]

    def ujson_leaves_get_caps(self, handles, cap_bytes, device=False, out=None):
        """one jy_ujson_leaves_get call with the given byte capacity ->
        ([bytes needed, handles not in the store], leaf_bytes, leaf_offs).  The
        outputs (numpy, or CUDA tensors with device=True; made here or passed as
        out = (bytes, offs)) are written only when cap_bytes is large enough."""
        h, ph, mh = _arg(handles, np.uint64)
        n, cap = len(h), int(cap_bytes)
        if out is not None:
            lb, lo = out
        elif device:
            import torch
            lb = torch.empty(max(cap, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
            lo = torch.empty(n + 1, dtype=torch.int64, device=f"cuda:{self.device}")
        else:
            lb, lo = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.uint64)
        assert len(lb) >= cap and len(lo) >= n + 1
        ptr = lambda a: C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)
        sizes = (C.c_uint64 * 2)()
        self._check(self.lib.jy_ujson_leaves_get(self.h, n, ph, mh, cap, ptr(lb), ptr(lo), sizes,
                                                 DEVICE if device else HOST))
        return [int(s) for s in sizes], lb, lo

    def ujson_leaves_get(self, handles, device=False):
        """the encoded leaves of `handles` (numpy, or a CUDA tensor) ->
        (leaf_bytes, leaf_offs[n + 1]); an unknown handle, and handle 0, give an
        empty item.  Two engine calls: one sizes, one fills.  Read-only."""
        need, _, _ = self.ujson_leaves_get_caps(handles, 0, device)
        sizes, lb, lo = self.ujson_leaves_get_caps(handles, need[0], device)
        assert sizes == need, (sizes, need)
        return lb[:need[0]], lo[:len(handles) + 1]

    def ujson_leaves_reserve(self, nleaves, nbytes):
        self._check(self.lib.jy_ujson_leaves_reserve(self.h, int(nleaves), int(nbytes)))

    def ujson_leaves_usage(self):
        """-> (leaves, arena bytes used, arena capacity, collisions)"""
        out = np.zeros(4, np.uint64)
        self._check(self.lib.jy_ujson_leaves_usage(self.h, out.ctypes.data))
        return tuple(int(x) for x in out)

    def ujson_leaves_collect(self, keep=None, shrink=False):
        """drop the leaves no document refers to (jy_ujson_leaves_collect): live
        are the elements of the state and of the pending deltas, and the
        handles in `keep` (numpy, or a CUDA tensor: leaves that were put and
        whose elements are not written yet).  shrink=True also brings table and
        arena down to 2 x what is kept.  -> LeavesCollected.  Synchronising.
        Refused, like arena_collect, while a router holds rounds in flight on
        this engine."""
        if getattr(self, "_route_holds", None):
            raise RuntimeError("ujson_leaves_collect while a router has rounds in flight on this engine: "
                               "call router.drain() first")
        if keep is None:
            n, pk, mk = 0, None, HOST
        else:
            k, pk, mk = _arg(keep, np.uint64)
            n = len(k)
        out = np.zeros(6, np.uint64)
        self._check(self.lib.jy_ujson_leaves_collect(self.h, n, pk, mk, _lib.LEAVES_SHRINK if shrink else 0,
                                                     out.ctypes.data))
        return LeavesCollected(*(int(x) for x in out))

    # -- UJSON path reads (jy_ujson_path_read): the elements at or under a path --
    def ujson_path_read_caps(self, slots, paths, leaves, cap_el, cap_bytes, device=False, out=None):
        """one jy_ujson_path_read call with the given capacities: query i = the
        live elements of document slots[i] (JY_NO_SLOT: no such key) whose leaf
        lies at or under paths[i] (a tuple of str) -> ([matched elements, leaf
        bytes, elements examined, examined handles not in the leaf store],
        {"el_offs", "elems", and with leaves "leaf_bytes", "leaf_offs"}).  The
        outputs (numpy, or CUDA tensors with device=True; made here or passed as
        `out`) are written only when both capacities are large enough."""
        from .ujson_doc import encode_path
        s = np.ascontiguousarray(slots, np.uint32)
        n, cap_el, cap_bytes = len(s), int(cap_el), int(cap_bytes)
        assert len(paths) == n
        enc = [encode_path(p) for p in paths]
        po = np.zeros(n + 1, np.uint64)
        po[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
        pb = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        shapes = [("el_offs", np.uint64, n + 1), ("elems", np.uint64, cap_el)]
        if leaves:
            shapes += [("leaf_bytes", np.uint8, cap_bytes), ("leaf_offs", np.uint64, cap_el + 1)]
        arrays = {}
        for name, dt, k in shapes:
            if out is not None:
                a = out[name]
                assert len(a) >= k, name
            elif device:
                import torch
                a = torch.empty(max(k, 1), dtype=getattr(torch, TORCH_DTYPE[dt]), device=f"cuda:{self.device}")
            else:
                a = np.zeros(max(k, 1), dt)
            arrays[name] = a
        ptr = lambda a: C.c_void_p(None if a is None else a.data_ptr() if _is_torch(a) else a.ctypes.data)
        sizes = (C.c_uint64 * 4)()
        self._check(self.lib.jy_ujson_path_read(
            self.h, n, s.ctypes.data, pb.ctypes.data, po.ctypes.data, _lib.PATH_LEAVES if leaves else 0, cap_el,
            cap_bytes, ptr(arrays["el_offs"]), ptr(arrays["elems"]), ptr(arrays.get("leaf_bytes")),
            ptr(arrays.get("leaf_offs")), sizes, DEVICE if device else HOST))
        return [int(x) for x in sizes], arrays

    def ujson_path_read(self, slots, paths, leaves=True, device=False):
        """the path reads of (slots[i], paths[i]) -> (sizes, el_offs[n + 1], elems,
        leaf_bytes, leaf_offs[matched + 1]) -- the last two None without leaves:
        per query the matched handles in converge order, and each one's encoding
        of (path relative to the query's, value).  Two engine calls: one sizes,
        one fills.  Read-only."""
        need, _ = self.ujson_path_read_caps(slots, paths, leaves, 0, 0, device)
        sizes, a = self.ujson_path_read_caps(slots, paths, leaves, need[0], need[1], device)
        assert sizes == need, (sizes, need)
        m = need[0]
        return (sizes, a["el_offs"][:len(slots) + 1], a["elems"][:m],
                a["leaf_bytes"][:need[1]] if leaves else None, a["leaf_offs"][:m + 1] if leaves else None)

    # -- keyed reads (jy_*_get_keys): GET by key string, answers in reply form --
    def _query(self, keys):
        """query keys -> (keepalive, key_bytes pointer, key_offs pointer, n, keys_mem):
        a list of str / bytes or a (bytes, offsets) pair of numpy arrays is host
        memory, a pair of CUDA tensors (uint8, int64) device memory"""
        if isinstance(keys, tuple) and _is_torch(keys[1]) and keys[1].is_cuda:
            kb, ko = keys
            assert kb.is_contiguous() and ko.is_contiguous() and ko.element_size() == 8
            return (kb, ko), C.c_void_p(kb.data_ptr()), C.c_void_p(ko.data_ptr()), int(ko.numel()) - 1, DEVICE
        kb, ko = self._keys(keys)
        return (kb, ko), C.c_void_p(kb.ctypes.data), C.c_void_p(ko.ctypes.data), len(ko) - 1, HOST

    def _outputs(self, shapes, device, out):
        """the output arrays of one call: (name, dtype, elements) each -- numpy
        zeros, CUDA tensors with device=True, or the caller's `out` (checked to
        be large enough) -> ({name: array}, [pointers])"""
        arrays, ptrs = {}, []
        for name, dt, k in shapes:
            if out is not None:
                a = out[name]
                assert len(a) >= k, name
            elif device:
                import torch
                a = torch.empty(max(k, 1), dtype=getattr(torch, TORCH_DTYPE[dt]), device=f"cuda:{self.device}")
            else:
                a = np.zeros(max(k, 1), dt)
            arrays[name] = a
            ptrs.append(C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data))
        return arrays, ptrs

    def _get_two_phase(self, kind, call, nsizes):
        """call(caps) -> (sizes, arrays), first with the capacities the last read
        of this kind needed: a steady caller makes ONE engine call, and only an
        answer that outgrew them a second one with the sizes the first reported"""
        memo = self.__dict__.setdefault("_get_caps", {})
        caps = memo.get(kind, [0] * nsizes)
        sizes, a = call(caps)
        if any(s > c for s, c in zip(sizes[:nsizes], caps)):
            need = sizes
            sizes, a = call(need[:nsizes])
            assert sizes == need, (sizes, need)
        if any(sizes[:nsizes]):
            memo[kind] = sizes[:nsizes]
        return sizes, a

    def treg_get_keys_caps(self, keys, cap_val_bytes, device=False, out=None):
        """one jy_treg_get_keys call with the given capacity -> ([value bytes,
        keys found], {"found", "ts", "val_bytes", "val_offs"}); the outputs are
        written only when the capacity is large enough"""
        hold, kb, ko, n, kmem = self._query(keys)
        cap = int(cap_val_bytes)
        a, p = self._outputs([("found", np.uint8, n), ("ts", np.uint64, n), ("val_bytes", np.uint8, cap),
                              ("val_offs", np.uint64, n + 1)], device, out)
        sizes = (C.c_uint64 * 2)()
        self._check(self.lib.jy_treg_get_keys(self.h, n, kb, ko, kmem, cap, *p, sizes, DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def treg_get_keys(self, keys, device=False):
        """TREG GET of a batch of keys (jy_treg_get_keys) -> {"found" u8[n], "ts"
        u64[n], "val_bytes", "val_offs" u64[n + 1], "sizes"}: a key never interned
        has found 0, ts 0 and an empty value.  Read-only; device=True: CUDA
        tensors, complete after sync()."""
        n = self._query(keys)[3]
        sizes, a = self._get_two_phase(("treg", bool(device)),
                                       lambda caps: self.treg_get_keys_caps(keys, caps[0], device), 1)
        return {"found": a["found"][:n], "ts": a["ts"][:n], "val_bytes": a["val_bytes"][:sizes[0]],
                "val_offs": a["val_offs"][:n + 1], "sizes": sizes}

    def tlog_get_keys_caps(self, keys, count, cap_ent, cap_val_bytes, device=False, out=None):
        """one jy_tlog_get_keys call with the given capacities -> ([entries, value
        bytes, keys found], {"found", "size", "cutoff", "ent_offs", "ts",
        "val_bytes", "val_offs"}); count: None (every entry) or one per key"""
        hold, kb, ko, n, kmem = self._query(keys)
        ce, cv = int(cap_ent), int(cap_val_bytes)
        cnt = None
        if count is not None:
            cnt = np.ascontiguousarray(count, np.uint64)
            assert len(cnt) == n
        a, p = self._outputs([("found", np.uint8, n), ("size", np.uint64, n), ("cutoff", np.uint64, n),
                              ("ent_offs", np.uint64, n + 1), ("ts", np.uint64, ce), ("val_bytes", np.uint8, cv),
                              ("val_offs", np.uint64, ce + 1)], device, out)
        sizes = (C.c_uint64 * 3)()
        self._check(self.lib.jy_tlog_get_keys(self.h, n, kb, ko, kmem, None if cnt is None else cnt.ctypes.data,
                                              ce, cv, *p, sizes, DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def tlog_get_keys(self, keys, count=None, device=False):
        """TLOG GET key [count] / SIZE / CUTOFF of a batch of keys
        (jy_tlog_get_keys) -> {"found" u8[n], "size" u64[n], "cutoff" u64[n],
        "ent_offs" u64[n + 1], "ts", "val_bytes", "val_offs" u64[entries + 1],
        "sizes"}: query i's min(size[i], count[i]) newest entries, newest first.
        count: None (every entry) or one per key (2^64 - 1: every entry; 0: none,
        which serves SIZE and CUTOFF).  Read-only; device=True: CUDA tensors,
        complete after sync()."""
        n = self._query(keys)[3]
        sizes, a = self._get_two_phase(("tlog", bool(device)),
                                       lambda caps: self.tlog_get_keys_caps(keys, count, caps[0], caps[1], device), 2)
        m = sizes[0]
        return {"found": a["found"][:n], "size": a["size"][:n], "cutoff": a["cutoff"][:n],
                "ent_offs": a["ent_offs"][:n + 1], "ts": a["ts"][:m], "val_bytes": a["val_bytes"][:sizes[1]],
                "val_offs": a["val_offs"][:m + 1], "sizes": sizes}

    def counter_get_keys(self, ctype, keys, device=False):
        """GCOUNT / PNCOUNT GET of a batch of keys (jy_counter_get_keys) ->
        (found u8[n], values: uint64 for GCOUNT, int64 for PNCOUNT); a missing key is 0"""
        hold, kb, ko, n, kmem = self._query(keys)
        a, p = self._outputs([("found", np.uint8, n), ("out", np.uint64, n)], device, None)
        self._check(self.lib.jy_counter_get_keys(self.h, ctype, n, kb, ko, kmem, *p, DEVICE if device else HOST))
        vals = a["out"][:n]
        if ctype == PNCOUNT and not device:
            vals = vals.view(np.int64)
        return a["found"][:n], vals

    # -- RESP replies (jy_*_get_resp): the keyed GETs answered as reply bytes --
    def _query_once(self, keys):
        """host keys encoded ONCE for the one or two calls of a two-phase read ->
        (the keys as _query takes them, n)"""
        if isinstance(keys, tuple) and _is_torch(keys[1]) and keys[1].is_cuda:
            return keys, int(keys[1].numel()) - 1
        kb, ko = self._keys(keys)
        return (kb, ko), len(ko) - 1

    def _resp_out(self, sizes, a, n):
        return {"reply_bytes": a["reply_bytes"][:sizes[0]], "reply_offs": a["reply_offs"][:n + 1], "sizes": sizes}

    def treg_get_resp_caps(self, keys, cap_bytes, device=False, out=None):
        """one jy_treg_get_resp call with the given capacity -> ([reply bytes, keys
        found], {"reply_bytes", "reply_offs"}); the outputs are written only when
        the capacity is large enough"""
        hold, kb, ko, n, kmem = self._query(keys)
        cap = int(cap_bytes)
        a, p = self._outputs([("reply_bytes", np.uint8, cap), ("reply_offs", np.uint64, n + 1)], device, out)
        sizes = (C.c_uint64 * 2)()
        self._check(self.lib.jy_treg_get_resp(self.h, n, kb, ko, kmem, cap, *p, sizes, DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def treg_get_resp(self, keys, device=False):
        """TREG GET of a batch of keys as RESP reply bytes (jy_treg_get_resp) ->
        {"reply_bytes", "reply_offs" u64[n + 1], "sizes"}: reply i is
        reply_bytes[reply_offs[i]:reply_offs[i + 1]], `$-1` for a key never
        interned.  Read-only; device=True: CUDA tensors, complete after sync()."""
        keys, n = self._query_once(keys)
        sizes, a = self._get_two_phase(("treg_resp", bool(device)),
                                       lambda caps: self.treg_get_resp_caps(keys, caps[0], device), 1)
        return self._resp_out(sizes, a, n)

    def tlog_get_resp_caps(self, keys, count, what, cap_bytes, device=False, out=None):
        """one jy_tlog_get_resp call with the given capacity -> ([reply bytes,
        entries, keys found], {"reply_bytes", "reply_offs"}); count: None (every
        entry) or one per key; what: None (GET) or one TLOG_RD_* per key"""
        hold, kb, ko, n, kmem = self._query(keys)
        cap = int(cap_bytes)
        cnt = wh = None
        if count is not None:
            cnt = np.ascontiguousarray(count, np.uint64)
            assert len(cnt) == n
        if what is not None:
            wh = np.ascontiguousarray(what, np.uint8)
            assert len(wh) == n
        a, p = self._outputs([("reply_bytes", np.uint8, cap), ("reply_offs", np.uint64, n + 1)], device, out)
        sizes = (C.c_uint64 * 3)()
        self._check(self.lib.jy_tlog_get_resp(self.h, n, kb, ko, kmem, None if wh is None else wh.ctypes.data,
                                              None if cnt is None else cnt.ctypes.data, cap, *p, sizes,
                                              DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def tlog_get_resp(self, keys, count=None, what=None, device=False):
        """TLOG GET key [count] / SIZE / CUTOFF of a batch of keys as RESP reply
        bytes (jy_tlog_get_resp) -> {"reply_bytes", "reply_offs" u64[n + 1],
        "sizes" [reply bytes, entries, keys found]}.  what: None (GET for every
        key) or TLOG_RD_GET / _SIZE / _CUTOFF per key; count as tlog_get_keys
        (SIZE and CUTOFF ignore it).  Read-only; device=True: CUDA tensors,
        complete after sync()."""
        keys, n = self._query_once(keys)
        sizes, a = self._get_two_phase(("tlog_resp", bool(device)),
                                       lambda caps: self.tlog_get_resp_caps(keys, count, what, caps[0], device), 1)
        return self._resp_out(sizes, a, n)

    def counter_get_resp_caps(self, ctype, keys, cap_bytes, device=False, out=None):
        """one jy_counter_get_resp call with the given capacity -> ([reply bytes,
        keys found], {"reply_bytes", "reply_offs"})"""
        hold, kb, ko, n, kmem = self._query(keys)
        cap = int(cap_bytes)
        a, p = self._outputs([("reply_bytes", np.uint8, cap), ("reply_offs", np.uint64, n + 1)], device, out)
        sizes = (C.c_uint64 * 2)()
        self._check(self.lib.jy_counter_get_resp(self.h, ctype, n, kb, ko, kmem, cap, *p, sizes,
                                                 DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def counter_get_resp(self, ctype, keys, device=False):
        """GCOUNT / PNCOUNT GET of a batch of keys as RESP reply bytes
        (jy_counter_get_resp) -> {"reply_bytes", "reply_offs" u64[n + 1], "sizes"}"""
        keys, n = self._query_once(keys)
        sizes, a = self._get_two_phase(("counter_resp", int(ctype), bool(device)),
                                       lambda caps: self.counter_get_resp_caps(ctype, keys, caps[0], device), 1)
        return self._resp_out(sizes, a, n)

    def ujson_get_resp_caps(self, keys, paths, cap_bytes, device=False, out=None):
        """one jy_ujson_get_resp call with the given capacity: query i = GET of
        keys[i] at paths[i] (tuples of str; paths=None: every path empty) ->
        ([reply bytes, keys found, distinct leaves rendered, elements examined,
        queries left to the host, examined handles not in the leaf store],
        {"reply_bytes", "reply_offs", "on_host"}); the outputs are written only
        when the capacity is large enough"""
        from .ujson_doc import encode_path
        hold, kb, ko, n, kmem = self._query(keys)
        cap = int(cap_bytes)
        pb = po = None
        if paths is not None:
            assert len(paths) == n
            enc = [encode_path(p) for p in paths]
            po = np.zeros(n + 1, np.uint64)
            po[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
            pb = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        a, p = self._outputs([("reply_bytes", np.uint8, cap), ("reply_offs", np.uint64, n + 1),
                              ("on_host", np.uint8, n)], device, out)
        sizes = (C.c_uint64 * 6)()
        self._check(self.lib.jy_ujson_get_resp(self.h, n, kb, ko, kmem, None if pb is None else pb.ctypes.data,
                                               None if po is None else po.ctypes.data, cap, *p, sizes,
                                               DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def ujson_get_resp(self, keys, paths=None, device=False):
        """UJSON GET key [path...] of a batch of (key, path) queries as RESP reply
        bytes, rendered on the device in stored order (jy_ujson_get_resp) ->
        {"reply_bytes", "reply_offs" u64[n + 1], "on_host" u8[n], "sizes"}:
        reply i is reply_bytes[reply_offs[i]:reply_offs[i + 1]], `$0` for a
        missing key or a path without leaves; on_host[i] = 1: the range is empty
        and the caller renders the query (ujson_doc.UJSONDocs.get_resp does).
        Read-only; device=True: CUDA tensors, complete after sync()."""
        keys, n = self._query_once(keys)
        sizes, a = self._get_two_phase(("ujson_resp", bool(device)),
                                       lambda caps: self.ujson_get_resp_caps(keys, paths, caps[0], device), 1)
        r = self._resp_out(sizes, a, n)
        r["on_host"] = a["on_host"][:n]
        return r

    # -- RESP requests (jy_resp_decode): client bytes decoded into keyed batches --
    RESP_SIZES = ("commands", "words", "rows", "key_bytes", "val_bytes", "groups")

    def _requests(self, conns):
        """connection buffers -> (keepalive, req pointer, req_mem, conn_offs, nconn):
        a list of bytes (joined here), or (bytes, conn_offs) with the bytes as
        bytes / a numpy uint8 array (host) or a CUDA uint8 tensor (device);
        conn_offs is always host memory"""
        if isinstance(conns, tuple):
            b, offs = conns
            offs = np.ascontiguousarray(offs, np.uint64)
        else:
            bs = [bytes(x) for x in conns]
            offs = np.zeros(len(bs) + 1, np.uint64)
            if bs:
                offs[1:] = np.cumsum([len(x) for x in bs], dtype=np.uint64)
            b = b"".join(bs)
        if _is_torch(b) and b.is_cuda:
            assert b.is_contiguous() and b.element_size() == 1
            return (b, offs), C.c_void_p(b.data_ptr()), DEVICE, offs, len(offs) - 1
        a = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b, np.uint8)
        return (a, offs), C.c_void_p(a.ctypes.data if len(a) else None), HOST, offs, len(offs) - 1

    @staticmethod
    def _resp_flags(ujson_get, ujson_write):
        return (_lib.RESP_UJSON_GET if ujson_get else 0) | (_lib.RESP_UJSON_WRITE if ujson_write else 0)

    def resp_decode_caps(self, conns, caps, device=False, out=None, ujson_get=False, opts=False, ujson_write=False):
        """one jy_resp_decode call with the given capacities (in the order of
        RESP_SIZES) -> (sizes, arrays); the arrays are written only when every
        capacity is large enough.  The group table is numpy whatever `device`.
        ujson_get=True: jy_resp_decode_opts with JY_RESP_UJSON_GET (opts=True:
        that entry point whatever the flags, 0 without ujson_get); ujson_write=True
        adds JY_RESP_UJSON_WRITE."""
        hold, preq, rmem, offs, nconn = self._requests(conns)
        cc, cw, cr, ck, cv, cg = caps = [int(x) for x in caps]
        a, p = self._outputs([("conn_used", np.uint64, nconn), ("conn_err", np.uint8, nconn),
                              ("cmd_conn", np.uint32, cc), ("cmd_kind", np.uint8, cc), ("cmd_phase", np.uint32, cc),
                              ("cmd_word_offs", np.uint64, cc + 1), ("word_off", np.uint64, cw),
                              ("word_len", np.uint64, cw), ("row_cmd", np.uint32, cr), ("key_bytes", np.uint8, ck),
                              ("key_offs", np.uint64, cr + 1), ("val_bytes", np.uint8, cv),
                              ("val_offs", np.uint64, cr + 1), ("num", np.uint64, cr), ("op", np.uint8, cr)],
                             device, out)
        g, pg = self._outputs([("group_phase", np.uint32, cg), ("group_class", np.uint8, cg),
                               ("group_offs", np.uint64, cg + 1)], False, out)
        a.update(g)
        ccaps = (C.c_uint64 * 6)(*caps)
        sizes = (C.c_uint64 * 6)()
        if ujson_get or ujson_write or opts:
            self._check(self.lib.jy_resp_decode_opts(self.h, nconn, preq, rmem, offs.ctypes.data, ccaps, *p, *pg, sizes,
                                                     DEVICE if device else HOST,
                                                     self._resp_flags(ujson_get, ujson_write)))
        else:
            self._check(self.lib.jy_resp_decode(self.h, nconn, preq, rmem, offs.ctypes.data, ccaps, *p, *pg, sizes,
                                                DEVICE if device else HOST))
        del hold
        return [int(x) for x in sizes], a

    def resp_decode(self, conns, device=False, ujson_get=False, ujson_write=False):
        """RESP requests decoded on the GPU (jy_resp_decode) -> a dict of the
        call's arrays cut to their sizes, plus "sizes": per connection conn_used
        / conn_err; per command cmd_conn, cmd_kind (CMD_*), cmd_phase and its
        words (cmd_word_offs into word_off / word_len, byte ranges of the
        request bytes); the keyed commands as rows sorted by (phase, kind) with
        key_bytes / key_offs, val_bytes / val_offs, num, op; and the host group
        table group_phase / group_class / group_offs.  conns: a list of
        connection buffers or (bytes, conn_offs).  The sizing call first, then
        the sized one, unless the capacities of the last decode still fit.
        ujson_get=True (JY_RESP_UJSON_GET): `UJSON GET key segment...` is a keyed
        kind too, CMD_UJSON_GET, whose value column is the path as
        ujson_doc.encode_path writes it, built on the device.
        ujson_write=True (JY_RESP_UJSON_WRITE): `UJSON INS / RM key segment...
        value` with a plain value and `UJSON CLR key` are the kind
        CMD_UJSON_WRITE: op = UJSON_INS / _RM / _CLR and the value column is the
        leaf as ujson_doc._encode writes it (empty for CLR), built on the device."""
        conns = self._requests(conns)[0]  # joined once for both calls
        nconn = len(conns[1]) - 1
        sizes, a = self._get_two_phase(("resp_decode", bool(device), bool(ujson_get), bool(ujson_write)),
                                       lambda caps: self.resp_decode_caps(conns, caps, device, ujson_get=ujson_get,
                                                                          ujson_write=ujson_write),
                                       6)
        nc, nw, nr, kb, vb, ng = sizes
        cut = {"conn_used": nconn, "conn_err": nconn, "cmd_conn": nc, "cmd_kind": nc, "cmd_phase": nc,
               "cmd_word_offs": nc + 1, "word_off": nw, "word_len": nw, "row_cmd": nr, "key_bytes": kb,
               "key_offs": nr + 1, "val_bytes": vb, "val_offs": nr + 1, "num": nr, "op": nr, "group_phase": ng,
               "group_class": ng, "group_offs": ng + 1}
        res = {name: a[name][:k] for name, k in cut.items()}
        res["sizes"] = sizes
        return res

    # -- RESP execute (jy_resp_exec / jy_resp_replies): request bytes to reply bytes --
    RESP_EXEC_SIZES = ("commands", "reply_bytes", "host_commands", "groups", "keyed_calls", "phases")
    RESP_EXEC_UJSON_SIZES = ("ujson_gets_on_device", "ujson_gets_on_host")  # [6], [7] with ujson_get=True

    def resp_exec_raw(self, conns, identity, on_host, ujson_get=False, ujson_write=False):
        """one jy_resp_exec call -> its sizes (in the order of RESP_EXEC_SIZES); the
        replies stay in the engine for resp_replies.  on_host(words) -> the reply
        of a command no keyed call exists for: bytes, or a list of byte pieces
        (each goes through jy_resp_sink_write); None: the batch may hold no such
        command.  An exception inside on_host fails the call and is raised again
        here once it has returned.  ujson_get=True: jy_resp_exec_opts with
        JY_RESP_UJSON_GET, eight sizes (RESP_EXEC_UJSON_SIZES follow); on_host
        then also answers the UJSON GETs the render leaves to the host.
        ujson_write=True: JY_RESP_UJSON_WRITE too (eight sizes): UJSON INS / RM /
        CLR groups are keyed writes on the device (ujson_write_keys_info has
        their counts)."""
        hold, preq, rmem, offs, nconn = self._requests(conns)
        raised = []

        def call(_ctx, _cmd, nwords, words, lens, sink):
            try:
                ans = on_host([C.string_at(words[j], lens[j]) for j in range(nwords)])
                for piece in ([ans] if isinstance(ans, (bytes, bytearray, memoryview)) else ans):
                    piece = bytes(piece)
                    if self.lib.jy_resp_sink_write(sink, piece, len(piece)) != 0:
                        raise EngineError(_lib.JY_EINVAL, "jy_resp_sink_write failed")
                return 0
            except BaseException as e:  # nothing may propagate through the C frames
                raised.append(e)
                return 1

        cb = _lib.RESP_HOST_FN(call) if on_host is not None else None
        pcb = C.cast(cb, C.c_void_p) if cb is not None else None
        if ujson_get or ujson_write:
            sizes = (C.c_uint64 * 8)()
            rc = self.lib.jy_resp_exec_opts(self.h, nconn, preq, rmem, offs.ctypes.data, int(identity), pcb, None,
                                            self._resp_flags(ujson_get, ujson_write), sizes)
        else:
            sizes = (C.c_uint64 * 6)()
            rc = self.lib.jy_resp_exec(self.h, nconn, preq, rmem, offs.ctypes.data, int(identity), pcb, None, sizes)
        del hold, cb
        if raised:
            raise raised[0]
        self._check(rc)
        return [int(x) for x in sizes]

    def resp_replies_caps(self, nconn, cap_bytes, device=False, out=None):
        """one jy_resp_replies call with the given capacity -> ([reply bytes,
        connections], {"reply_bytes", "conn_reply_offs", "conn_used", "conn_err"});
        the arrays are written only when the capacity is large enough"""
        cap = int(cap_bytes)
        a, p = self._outputs([("reply_bytes", np.uint8, cap), ("conn_reply_offs", np.uint64, nconn + 1),
                              ("conn_used", np.uint64, nconn), ("conn_err", np.uint8, nconn)], device, out)
        sizes = (C.c_uint64 * 2)()
        self._check(self.lib.jy_resp_replies(self.h, nconn, cap, *p, sizes, DEVICE if device else HOST))
        return [int(x) for x in sizes], a

    def resp_exec(self, conns, identity, on_host, device=False, ujson_get=False, ujson_write=False):
        """The receive buffers of a heartbeat's connections decoded, applied and
        answered in one engine call (jy_resp_exec), the replies assembled per
        connection on the GPU; the reference is jylis_amd.resp_in.exec_resp.
        conns: a list of connection buffers or (bytes, conn_offs), as resp_decode.
        -> one (reply bytes, bytes consumed, closed) per connection; with
        device=True the raw arrays as CUDA tensors (complete after sync()):
        {"reply_bytes", "conn_reply_offs" u64[nconn + 1], "conn_used", "conn_err",
        "sizes": the call's six, by RESP_EXEC_SIZES}.  ujson_get=True: UJSON GET
        is decoded and rendered on the device too (jy_resp_exec_opts; the caller
        holds the leaf store's lock, as ujson_doc.UJSONDocs.resp_exec does).
        ujson_write=True: UJSON INS / RM / CLR are keyed writes on the device too,
        under the same lock."""
        conns = self._requests(conns)[0]
        nconn = len(conns[1]) - 1
        sizes = self.resp_exec_raw(conns, identity, on_host, ujson_get=ujson_get, ujson_write=ujson_write)
        got, a = self.resp_replies_caps(nconn, sizes[1], device)
        assert got == [sizes[1], nconn], (got, sizes)
        if device:
            return {"reply_bytes": a["reply_bytes"][:sizes[1]], "conn_reply_offs": a["conn_reply_offs"][:nconn + 1],
                    "conn_used": a["conn_used"][:nconn], "conn_err": a["conn_err"][:nconn], "sizes": sizes}
        rb, ro = a["reply_bytes"].tobytes(), a["conn_reply_offs"].astype(np.int64)
        return [(rb[ro[c]:ro[c + 1]], int(a["conn_used"][c]), bool(a["conn_err"][c])) for c in range(nconn)]

    def with_leaves(self, ctype, w, device=False):
        """a UJSON wire batch plus leaf_bytes / leaf_offs[nel + 1], parallel to its
        `elems` (one item per element, not de-duplicated): jy_ujson_leaves_get on
        the batch's elems, on the device for a device batch.  Other types: w."""
        if ctype != UJSON:
            return w
        out = dict(w)
        out["leaf_bytes"], out["leaf_offs"] = self.ujson_leaves_get(w["elems"], device)
        return out

    # -- state snapshot in wire form (jy_*_state_wire): state as a converge batch --
    def state_wire_caps(self, ctype, slot0, nslots, caps, device=False, out=None):
        """one jy_*_state_wire call over the slots [slot0, slot0 + nslots) with the
        given output capacities (WIRE_SIZES[ctype] order; caps[0] is not passed: the
        per-key arrays always hold nslots elements) -> (sizes needed, {name: array}).
        The arrays are those of flush_wire_caps (WIRE_ARRAYS[ctype]), made here or
        passed as `out`; they are filled only when no capacity is short.  Device
        outputs are complete after sync().  A range outside the interned keys raises
        EngineError (JY_ERANGE) and writes nothing."""
        head = ([ctype] if ctype in (GCOUNT, PNCOUNT) else []) + [int(slot0), int(nslots)]
        return self._wire_call(_STATE_WIRE_FN[ctype], ctype, head, [nslots, *caps[1:]], False, device, out)

    def state_wire(self, ctype, slot0, nslots, device=False, leaves=False):
        """the state of the slots [slot0, slot0 + nslots) as the arrays the type's
        jy_node_*_converge takes ({name: array}, as flush_wire): one record per
        slot, in slot order, bottom-state slots included.  Two engine calls: one
        sizes the range, one fills it.  Read-only.  leaves=True: as flush_wire."""
        return self._wire_two_phase(ctype, lambda caps: self.state_wire_caps(ctype, slot0, nslots, caps, device),
                                    device, leaves)

    # -- state digest in key-hash buckets, and the repair path built on it --
    def digest_range(self, ctype, nbuckets, slot0, nslots, device=False):
        """one jy_*_state_digest call: the [nbuckets, 4] rows {digest, keys, items,
        bytes-or-cloud} of the slots [slot0, slot0 + nslots) (numpy uint64, or an
        int64 CUDA tensor with device=True, complete after sync()).  Read-only."""
        nb = int(nbuckets)
        if device:
            import torch
            out = torch.empty((max(nb, 1), 4), dtype=torch.int64, device=f"cuda:{self.device}")
            ptr = out.data_ptr()
        else:
            out = np.zeros((max(nb, 1), 4), np.uint64)
            ptr = out.ctypes.data
        fn = getattr(self.lib, _DIGEST_FN[ctype])
        head = [ctype] if ctype in (GCOUNT, PNCOUNT) else []
        self._check(fn(self.h, *head, int(slot0), int(nslots), nb, C.c_void_p(ptr), DEVICE if device else HOST))
        return out

    def digest(self, ctype, nbuckets=1, slot0=0, nslots=None, max_keys=65536, device=False):
        """the canonical state digest of the slots [slot0, slot0 + nslots) (default:
        every key of the type) split into `nbuckets` key-hash buckets: a [B, 4]
        uint64 array, row b = {digest, keys, items, bytes-or-cloud} of bucket b.
        It depends on neither slot, column nor key order: engines that hold the
        same data give the same array, and rows add up (wrapping) over chunks and
        shards.  The range is read in chunks of max_keys slots summed with a
        wrapping add, so the TLOG / UJSON temporaries stay bounded."""
        n = self.nkeys(ctype) - int(slot0) if nslots is None else int(nslots)
        if n <= int(max_keys):  # (also the calls that must fail: the engine reports them)
            return self.digest_range(ctype, nbuckets, slot0, n, device)
        total = None
        for s0 in range(int(slot0), int(slot0) + n, int(max_keys)):
            d = self.digest_range(ctype, nbuckets, s0, min(int(max_keys), int(slot0) + n - s0), device)
            if total is None:
                total = d
            elif device:
                import torch
                self.sync()  # d is complete ...
                total += d  # (int64 adds wrap like uint64)
                # ... and the add has run before the engine's stream may write memory torch hands out again
                torch.cuda.current_stream(self.device).synchronize()
            else:
                with np.errstate(over="ignore"):
                    total += d
        return total

    def bucket_slots(self, ctype, nbuckets, buckets, slot0=0, nslots=None):
        """the slots of [slot0, slot0 + nslots) (default: every key) whose key falls
        into one of `buckets` (indices below nbuckets), ascending (uint32)"""
        nb = int(nbuckets)
        n = self.nkeys(ctype) - int(slot0) if nslots is None else int(nslots)
        bits = np.zeros((max(nb, 1) + 63) // 64, np.uint64)
        for b in np.asarray(buckets, np.int64).ravel().tolist():
            if not 0 <= b < nb:
                raise ValueError(f"bucket {b} is outside [0, {nb})")
            bits[b >> 6] |= np.uint64(1 << (b & 63))
        k = C.c_uint64(0)
        call = lambda cap, out: self._check(self.lib.jy_state_bucket_slots(
            self.h, ctype, int(slot0), n, nb, bits.ctypes.data, cap, out, C.byref(k), HOST))
        call(0, None)
        out = np.zeros(max(int(k.value), 1), np.uint32)
        if k.value:
            call(int(k.value), out.ctypes.data)
        return out[:int(k.value)]

    def state_wire_slots_caps(self, ctype, slots, caps, device=False, out=None):
        """one jy_*_state_wire_slots call: state_wire_caps for a strictly ascending
        slot list (a host array) instead of a range"""
        slots = np.ascontiguousarray(slots, np.uint32)
        head = ([ctype] if ctype in (GCOUNT, PNCOUNT) else []) + [len(slots), C.c_void_p(slots.ctypes.data), HOST]
        return self._wire_call(_STATE_WIRE_FN[ctype] + "_slots", ctype, head, [len(slots), *caps[1:]], False, device,
                               out)

    def state_wire_slots(self, ctype, slots, device=False, leaves=False):
        """the state of the listed slots (strictly ascending, all interned) as a wire
        batch: record i is the state of slots[i].  Two engine calls, as state_wire."""
        return self._wire_two_phase(ctype, lambda caps: self.state_wire_slots_caps(ctype, slots, caps, device),
                                    device, leaves)

    def snapshot(self, ctype, max_keys=65536, device=False, leaves=False):
        """the whole state of one type as wire batches over [0, keys_count), at
        most max_keys slots each, in slot order (a generator: one chunk is
        resident at a time; nothing for an empty type)"""
        n = self.nkeys(ctype)
        for s0 in range(0, n, int(max_keys)):
            yield self.state_wire(ctype, s0, min(int(max_keys), n - s0), device, leaves)

    def converge_wire(self, ctype, w):
        """one wire batch (host arrays: state_wire's, flush_wire's) into this engine,
        the way the GPU-backed repos converge a decoded batch: the keys are interned
        in batch order (so a snapshot re-creates its key directory), TREG / TLOG
        values are packed into the arena, then the type's converge call runs.
        Columns are this engine's.  A UJSON batch that carries leaf_bytes /
        leaf_offs has its leaves put into the leaf store FIRST; the handles the
        store derives must equal the batch's elems, else EngineError is raised and
        nothing is converged."""
        a = {name: np.asarray(w[name], dt) for name, dt, _, _ in WIRE_ARRAYS[ctype]}
        keys = (a["key_bytes"], a["key_offs"])
        n = len(a["key_offs"]) - 1
        if n <= 0:
            return
        if ctype == UJSON and has_leaves(w):
            self.put_wire_leaves(a["elems"], w["leaf_bytes"], w["leaf_offs"])
        if ctype in (GCOUNT, PNCOUNT):
            if len(a["col"]) == 0:
                self.intern(ctype, keys)  # converge creates the keys (_data_for) even with no cells
                return
            cell_key = np.repeat(np.arange(n, dtype=np.uint32), np.diff(a["cell_offs"]).astype(np.int64))
            self.counter_converge_keys(ctype, keys, a["col"], a["val"], cell_key=cell_key,
                                       sign=a["sign"] if ctype == PNCOUNT else None)
            return
        slots = self.intern(ctype, keys)
        if ctype == TREG:
            pre, lr = self.pack_values(TREG, (a["val_bytes"], a["val_offs"]))
            self.treg_converge(slots, a["ts"], pre, lr)
        elif ctype == TLOG:
            pre, lr = self.pack_values(TLOG, (a["val_bytes"], a["val_offs"]))
            self.tlog_converge(slots, a["cutoff"], a["ent_offs"], a["ts"], pre, lr)
        elif ctype == UJSON:
            self.ujson_converge(slots, a["el_offs"], a["dots"], a["elems"], a["vv_offs"], a["vv"], a["cloud_offs"],
                                a["cloud"])
        else:
            raise ValueError(f"unknown CRDT type {ctype}")

    def put_wire_leaves(self, elems, leaf_bytes, leaf_offs):
        """the leaves of a UJSON wire batch (host arrays) into the leaf store,
        checked against the batch's elems"""
        elems = np.asarray(elems, np.uint64)
        lo = np.asarray(leaf_offs, np.uint64)
        if len(lo) != len(elems) + 1:
            raise EngineError(_lib.JY_EINVAL, f"leaf_offs has {len(lo)} entries for {len(elems)} elements")
        if len(elems) == 0:
            return
        got = self.ujson_leaves_put(np.asarray(leaf_bytes, np.uint8), lo)
        bad = np.nonzero(got != elems)[0]
        if len(bad):
            i = int(bad[0])
            raise EngineError(_lib.JY_EINVAL, f"{len(bad)} leaves of a UJSON batch do not hash to their elements "
                                              f"(first: item {i}, element {int(elems[i]):#x}, leaf {int(got[i]):#x})")

    def counter_state_mask_rows(self):
        """rows (signs x columns) up to which the counter snapshot's tile writer runs"""
        return int(self.lib.jy_counter_state_mask_rows())


# the wire-form flush's outputs per type: the capacity / size names in call
# order, and (array, dtype, index of its size, extra elements) in call order --
# the argument order of the type's jy_node_*_converge after the count
_COUNTER_WIRE = (("key_bytes", np.uint8, 1, 0), ("key_offs", np.uint64, 0, 1), ("cell_offs", np.uint64, 0, 1),
                 ("sign", np.uint8, 2, 0), ("col", np.uint16, 2, 0), ("val", np.uint64, 2, 0))
WIRE_SIZES = {
    GCOUNT: ("keys", "key_bytes", "cells"),
    PNCOUNT: ("keys", "key_bytes", "cells"),
    TREG: ("keys", "key_bytes", "val_bytes"),
    TLOG: ("keys", "key_bytes", "entries", "val_bytes"),
    UJSON: ("docs", "key_bytes", "elements", "vv", "cloud"),
}
WIRE_ARRAYS = {
    GCOUNT: _COUNTER_WIRE,
    PNCOUNT: _COUNTER_WIRE,
    TREG: (("key_bytes", np.uint8, 1, 0), ("key_offs", np.uint64, 0, 1), ("ts", np.uint64, 0, 0),
           ("val_bytes", np.uint8, 2, 0), ("val_offs", np.uint64, 0, 1)),
    TLOG: (("key_bytes", np.uint8, 1, 0), ("key_offs", np.uint64, 0, 1), ("cutoff", np.uint64, 0, 0),
           ("ent_offs", np.uint64, 0, 1), ("ts", np.uint64, 2, 0), ("val_bytes", np.uint8, 3, 0),
           ("val_offs", np.uint64, 2, 1)),
    UJSON: (("key_bytes", np.uint8, 1, 0), ("key_offs", np.uint64, 0, 1), ("el_offs", np.uint64, 0, 1),
            ("dots", np.uint64, 2, 0), ("elems", np.uint64, 2, 0), ("vv_offs", np.uint64, 0, 1),
            ("vv", np.uint64, 3, 0), ("cloud_offs", np.uint64, 0, 1), ("cloud", np.uint64, 4, 0)),
}
# the torch dtype (by name: torch is imported only for device outputs) that holds
# each numpy dtype of the wire arrays.  torch has no unsigned 16 / 64: the same
# widths, signed
TORCH_DTYPE = {np.uint8: "uint8", np.uint16: "int16", np.uint32: "int32", np.uint64: "int64"}
# arrays a wire batch MAY carry besides WIRE_ARRAYS (name, dtype): they are no
# argument of the wire calls (WIRE_ARRAYS stays the calls' argument list) but
# derived from the batch -- a UJSON batch's leaves, parallel to its `elems`
# (Engine.with_leaves), leaf_offs one longer than elems
WIRE_OPTIONAL = {
    GCOUNT: (), PNCOUNT: (), TREG: (), TLOG: (),
    UJSON: (("leaf_bytes", np.uint8), ("leaf_offs", np.uint64)),
}


def has_leaves(w):
    """the wire batch carries both leaf arrays"""
    return "leaf_bytes" in w and "leaf_offs" in w


_WIRE_FN = {GCOUNT: "jy_counter_flush_wire", PNCOUNT: "jy_counter_flush_wire", TREG: "jy_treg_flush_wire",
            TLOG: "jy_tlog_flush_wire", UJSON: "jy_ujson_flush_wire"}
_DIGEST_FN = {GCOUNT: "jy_counter_state_digest", PNCOUNT: "jy_counter_state_digest", TREG: "jy_treg_state_digest",
              TLOG: "jy_tlog_state_digest", UJSON: "jy_ujson_state_digest"}
_STATE_WIRE_FN = {GCOUNT: "jy_counter_state_wire", PNCOUNT: "jy_counter_state_wire", TREG: "jy_treg_state_wire",
                  TLOG: "jy_tlog_state_wire", UJSON: "jy_ujson_state_wire"}


def key_owner(key, nshards):
    lib = _lib.load()
    b = key.encode() if isinstance(key, str) else bytes(key)
    buf = C.create_string_buffer(b, len(b) or 1)
    return int(lib.jy_key_owner(buf, len(b), nshards))
