"""UJSON documents above the dot kernel: paths, JSON leaves and rendering.

Mirrors RepoUJSON's command surface (repo_ujson.pony:68-110) and the UJSON
data model of docs/_docs/types/ujson.md:134-170 ("the world is flat"): a
document is a set of (path, value) leaves, each an element of the engine's
observed-remove dot kernel.  The engine stores elements as opaque u64
handles; this module owns the mapping.

  GET key [path...]         render the leaves at or under path ('' if none)
  SET key [path...] ujson   CLR path, then INS every leaf of the parsed node
  CLR key [path...]         remove every leaf at or under path (no key creation)
  INS key [path...] value   add the leaf (path, value)
  RM  key [path...] value   remove the leaf (path, value) (no key creation)

Handles are a 64-bit hash (FNV-1a) of the canonical (path, value) encoding
(each path segment length-prefixed, then 0xFFFFFFFF, then the value), so every
replica derives the same handle for the same leaf (the CRDT compares elements
by handle); `LeafTable` keeps handle -> leaf for rendering and refuses a hash
collision.  Rendering follows the primer: maps render as objects, several
values at one path as an unordered set '[...]', one value bare, at most one
merged map inside a set, nothing for empty collections.  Set and map order is
not specified by the reference (pony Map iteration); `render` writes keys
and set members in sorted order, `render_stored_order` in the order of the
leaves' stored bytes (the device's, jy_ujson_get_resp), and tests compare
renders canonically (`canonical`)."""
import contextlib
import json
import threading

import numpy as np


def canonical_value(text):
    """a UJSON primitive (UJSONParse.value) -> its canonical JSON text"""
    v = json.loads(text)
    if isinstance(v, (dict, list)):
        raise ValueError("a UJSON value is a primitive (string, number, boolean, null)")
    return _dump(v)


def _dump(v):
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return json.dumps(v, ensure_ascii=False)
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return repr(v)
    raise ValueError(f"not a JSON primitive: {v!r}")


def flatten(text, prefix=()):
    """UJSONParse.node: a JSON document -> set of (path, canonical value)
    leaves; arrays are sets (flattened into the enclosing path)"""
    out = set()

    def walk(v, path):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(x, path + (str(k),))
        elif isinstance(v, list):
            for x in v:
                walk(x, path)
        else:
            out.add((path, _dump(v)))
    walk(json.loads(text), tuple(prefix))
    return out


def _fnv1a64(b):
    h = 0xCBF29CE484222325
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def encode_path(path):
    """a path's segments as a leaf encoding carries them, without the
    terminator: a byte prefix of _encode(q, v) iff `path` is a prefix of q
    (what jy_ujson_path_read compares on the device)"""
    b = bytearray()
    for p in path:
        e = bytes(p) if isinstance(p, (bytes, bytearray)) else p.encode()
        b += len(e).to_bytes(4, "little") + e
    return bytes(b)


def _encode(path, value):
    return encode_path(path) + b"\xff\xff\xff\xff" + value.encode()


class LeafTable:
    """(path, value) <-> u64 handle; one table serves every replica of a process"""

    def __init__(self):
        self._leaf = {}

    def handle(self, path, value):
        path = tuple(path)
        # FNV-1a 64 of the encoding (the Pony glue computes the same handle);
        # handle 0 is reserved: "no element" (the engine's key-touching RM)
        h = _fnv1a64(_encode(path, value)) or 1
        old = self._leaf.setdefault(h, (path, value))
        if old != (path, value):
            raise RuntimeError(f"64-bit leaf handle collision: {old} vs {(path, value)}")
        return h

    def leaf(self, h):
        return self._leaf[int(h)]


def _decode(b):
    """_encode's inverse: the encoding's bytes -> (path, value)"""
    b = bytes(b)
    path, at = [], 0
    while True:
        if at + 4 > len(b):
            raise ValueError("a leaf encoding ends before its terminator")
        n = int.from_bytes(b[at:at + 4], "little")
        at += 4
        if n == 0xFFFFFFFF:
            return tuple(path), b[at:].decode()
        if at + n > len(b):
            raise ValueError("a leaf encoding's path segment reaches past its end")
        path.append(b[at:at + n].decode())
        at += n


class DeviceLeaves:
    """LeafTable's interface over an engine's device leaf store
    (jy_ujson_leaves_*): the leaves live in HBM next to the documents, so wire
    batches can carry them (flush_wire / state_wire / snapshot with
    leaves=True) and a process that received such a batch can render it.
    `lock`: a callable giving a context manager held around each engine call
    (a node's shard: lambda: node.locked(UJSON)); lock() takes it, once per
    thread however the calls nest.
    The store only grows between collections.  collect() drops the leaves no
    document refers to; with auto_collect=True UJSONDocs calls maybe_collect()
    after each write command, which collects by the arena policy of repo.py
    (_ArenaGC): when the arena bytes in use exceed 2 x the bytes the last
    collection kept + `floor`.  `collections` counts the collections run."""

    def __init__(self, engine, lock=None, auto_collect=False, floor=1 << 20):
        self.eng = engine
        self._lock = lock if lock is not None else contextlib.nullcontext
        self._held = threading.local()  # how deep THIS thread is inside lock()
        self.auto_collect = bool(auto_collect)
        self.floor = int(floor)
        self.collections = 0
        self._kept_bytes = 0  # arena bytes the last collection kept

    @contextlib.contextmanager
    def lock(self):
        """the constructor's lock, re-entrant for the thread that holds it: a
        call made under it (UJSONDocs.resp_exec holds it for a whole heartbeat,
        and its callback reads and writes leaves) enters without taking it
        again; every other thread waits for it as before"""
        depth = getattr(self._held, "n", 0)
        if depth:
            self._held.n = depth + 1
            try:
                yield
            finally:
                self._held.n = depth
            return
        with self._lock():
            self._held.n = 1
            try:
                yield
            finally:
                self._held.n = 0

    def collect(self, keep=(), shrink=False):
        """Engine.ujson_leaves_collect under the lock.  `keep`: handles that
        handle() returned and no write command has used yet."""
        keep = np.asarray(list(keep), np.uint64) if not hasattr(keep, "data_ptr") else keep
        with self.lock():
            got = self.eng.ujson_leaves_collect(keep if len(keep) else None, shrink)
        self.collections += 1
        self._kept_bytes = got.kept_bytes
        return got

    def maybe_collect(self, floor=None):
        """collect() if the arena holds more than 2 x what the last collection
        kept + floor bytes -> its result, else None.  Reads the usage, which
        waits for the stream: call it after a write command, whose puts have
        blocked already, and when every handle put so far is in a document or
        a pending delta (no `keep`)."""
        floor = self.floor if floor is None else int(floor)
        with self.lock():
            used = self.eng.ujson_leaves_usage()[1]
        if used <= 2 * self._kept_bytes + floor:
            return None
        return self.collect()

    def handle(self, path, value):
        enc = np.frombuffer(_encode(tuple(path), value), np.uint8)
        with self.lock():
            h = int(self.eng.ujson_leaves_put(enc, np.array([0, len(enc)], np.uint64))[0])
        if h == 0:
            raise RuntimeError(f"the leaf store refused {(tuple(path), value)}: a 64-bit leaf handle collision "
                               "(or a leaf longer than 16 MiB)")
        return h

    def leaves(self, handles):
        """[(path, value)] of many handles with one engine read; KeyError for an unknown one"""
        hs = np.asarray(list(handles), np.uint64)
        if len(hs) == 0:
            return []
        with self.lock():
            lb, lo = self.eng.ujson_leaves_get(hs)
        raw, lo = lb.tobytes(), lo.astype(np.int64)
        out = []
        for i, h in enumerate(hs):
            if lo[i + 1] == lo[i]:
                raise KeyError(int(h))
            out.append(_decode(raw[lo[i]:lo[i + 1]]))
        return out

    def leaf(self, h):
        return self.leaves([int(h)])[0]

    def under(self, slots, paths, leaves=True):
        """per query (slots[i], paths[i]): [(handle, (relative path, value))] of
        the document's live elements at or under the path, selected on the
        device with one path read (jy_ujson_path_read); leaves=False: the
        handles alone.  KeyError if an element's leaf is not in the store."""
        with self.lock():
            sizes, eo, elems, lb, lo = self.eng.ujson_path_read(slots, paths, leaves)
        if sizes[3]:
            raise KeyError(f"{sizes[3]} element(s) of the documents read have no leaf in the store")
        eo, hs = eo.astype(np.int64), elems.tolist()
        if leaves:
            raw, lo = lb.tobytes(), lo.astype(np.int64)
            hs = [(h, _decode(raw[lo[j]:lo[j + 1]])) for j, h in enumerate(hs)]
        return [hs[eo[i]:eo[i + 1]] for i in range(len(slots))]


def render(leaves):
    """leaves [(relative path, value)] -> UJSON text ('' when empty)"""
    if not leaves:
        return ""
    root = {"v": set(), "m": {}}
    for path, value in leaves:
        n = root
        for p in path:
            n = n["m"].setdefault(p, {"v": set(), "m": {}})
        n["v"].add(value)

    def out(n):
        items = sorted(n["v"])
        m = {k: c for k, c in n["m"].items() if _nonempty(c)}
        if m:
            items.append("{" + ",".join(json.dumps(k, ensure_ascii=False) + ":" + out(m[k]) for k in sorted(m)) + "}")
        if len(items) == 1:
            return items[0]
        return "[" + ",".join(items) + "]"
    return out(root)


def render_stored_order(leaves):
    """leaves [(relative path, value)] -> UJSON text in STORED ORDER ('' when
    empty): the one order the device render uses (jy_ujson_get_resp,
    csrc/jy_uj_render.hpp), stated here once for the host.

    The distinct encodings _encode(path, value) are sorted as bytes, a proper
    prefix first.  Under a node that puts its children first, by the bytes of
    their encoded segment (the four little-endian length bytes, then the key),
    and the node's own values after them by the bytes of their text; all
    leaves under a node are contiguous.  A node's items are {"k":<child>,...}
    if it has children, then each value verbatim; one item renders bare,
    several as [item,item,...]; keys go between quotes verbatim.  The text is
    written leaf by leaf from that order -- no tree is built -- each leaf
    owning the punctuation before and after it.  The one fact a leaf cannot
    see from its neighbours, whether a node it opens through a child also has
    values of its own (they lie at the END of the node's range), is carried
    right to left as a set of levels."""
    order = sorted({_encode(tuple(p), v): (tuple(p), v) for p, v in leaves}.items())
    items = [leaf for _, leaf in order]
    k = len(items)
    if k == 0:
        return ""

    def shared(a, b):
        n = 0
        while n < len(a) and n < len(b) and a[n] == b[n]:
            n += 1
        return n

    # state[j]: the levels t whose node on leaf j's path has own values at or right of j
    state, cur = [0] * k, 0
    for j in range(k - 1, -1, -1):
        keep = 0 if j == k - 1 else shared(items[j][0], items[j + 1][0]) + 1
        cur = (cur & ((1 << keep) - 1)) | (1 << len(items[j][0]))
        state[j] = cur
    out = []
    for j, (path, value) in enumerate(items):
        first, last, d = j == 0, j == k - 1, len(path)
        cp = 0 if first else shared(items[j - 1][0], path)
        cs = 0 if last else shared(path, items[j + 1][0])
        dnext = 0 if last else len(items[j + 1][0])
        kfirst = 1 if first else cp + 1
        after_key = False
        for seg in range(kfirst, d + 1):
            if after_key:
                out.append('":')
            if not first and seg == kfirst:
                out.append(",")  # a further child of the node at level cp
            else:  # the node at level seg - 1 opens here through this child
                out.append("[{" if state[j] >> (seg - 1) & 1 else "{")
            out.append('"' + path[seg - 1])
            after_key = True
        if after_key:
            out.append('":')
        opens = first or d > cp  # its own node opens with this value
        if not opens:
            out.append(",")
        elif not last and cs == d and dnext == d:
            out.append("[")
        out.append(value)
        ends = last or cs < d
        if ends and not first and cp == d:
            out.append("]")
        lo = 0 if last else cs + 1
        nb = max(0, d - lo)
        if not last and d > cs and dnext == cs:
            nb += 1  # the successor is a value of the node at level cs
        out.append("}" * nb)
    return "".join(out)


def _nonempty(n):
    return bool(n["v"]) or any(_nonempty(c) for c in n["m"].values())


def canonical(text):
    """a UJSON render -> a comparable structure (sets and maps unordered)"""
    if text == "":
        return None

    def canon(v):
        if isinstance(v, dict):
            return ("map", frozenset((k, canon(x)) for k, x in v.items()))
        if isinstance(v, list):
            flat = set()
            maps = {}
            for x in v:
                c = canon(x)
                if c[0] == "set":
                    flat |= c[1]
                elif c[0] == "map":
                    maps.update(dict(c[1]))
                else:
                    flat.add(c)
            if maps:
                flat.add(("map", frozenset(maps.items())))
            return ("set", frozenset(flat)) if len(flat) != 1 else next(iter(flat))
        return ("val", _dump(v))
    return canon(json.loads(text))


class UJSONDocs:
    """RepoUJSON's commands over a dot-kernel backend (the GPU RepoUJSON, or
    the oracle in tests).  backend: write(cmds, identity) with ("INS", key,
    h) / ("RM", key, h) / ("CLR", key) / ("TOUCH", key) (create the key and
    its delta, change nothing); elements(keys) -> {key: [handles]};
    exists(key)."""

    def __init__(self, backend, identity, leaves=None):
        self.b = backend
        self.identity = identity
        self.leaves = leaves if leaves is not None else LeafTable()

    def _written(self):
        """after a write command has returned: every handle it put is in the
        state or the pending delta, so an auto-collecting leaf store may drop
        what nothing refers to (DeviceLeaves.maybe_collect)"""
        if getattr(self.leaves, "auto_collect", False):
            self.leaves.maybe_collect()

    def _leaves_of(self, handles):
        """{handle: (path, value)}: one batched read where the table offers
        leaves(handles) (DeviceLeaves: one engine call), else one leaf() each"""
        hs = sorted(set(int(x) for x in handles))
        if hasattr(self.leaves, "leaves"):
            return dict(zip(hs, self.leaves.leaves(hs)))
        return {h: self.leaves.leaf(h) for h in hs}

    def _device_paths(self):
        """the leaves object selects by path on the device (DeviceLeaves.under)
        and the backend's documents live in the same engine"""
        return hasattr(self.leaves, "under") and isinstance(self.b, GpuDocs) and \
            getattr(self.leaves, "eng", None) is self.b.r.eng

    def _under(self, key, path):
        path = tuple(path)
        if self._device_paths():
            return set(self.leaves.under(self.b.r.slots_of([key]), [path], leaves=False)[0])
        hs = self.b.elements([key]).get(key, [])
        out = set()
        for h, (p, v) in self._leaves_of(hs).items():
            if p[:len(path)] == path:
                out.add(h)
        return out

    def get(self, key, path=()):
        """GET (repo_ujson.pony:68-72)"""
        return self.get_many([key], path)[0]

    def get_many(self, keys, path=()):
        """GET for many docs with one engine read"""
        path = tuple(path)
        if self._device_paths():
            return self.get_paths(keys, [path] * len(keys))
        els = self.b.elements(list(keys))
        known = self._leaves_of(h for k in keys for h in els.get(k, []))
        out = []
        for k in keys:
            leaves = []
            for h in set(int(x) for x in els.get(k, [])):
                p, v = known[h]
                if p[:len(path)] == path:
                    leaves.append((p[len(path):], v))
            out.append(render(leaves))
        return out

    def get_paths(self, keys, paths):
        """GET of keys[i] at paths[i], with one engine read"""
        keys, paths = list(keys), [tuple(p) for p in paths]
        if not keys:
            return []
        if not self._device_paths():
            return [self.get_many([k], p)[0] for k, p in zip(keys, paths)]
        found = self.leaves.under(self.b.r.slots_of(keys), paths, leaves=True)
        return [render(list(set(leaf for _, leaf in q))) for q in found]

    def get_resp(self, keys, paths):
        """GET of keys[i] at paths[i] as RESP reply bytes -> [bytes]: reply i is
        `$<len>\\r\\n<text>\\r\\n` with the text in stored order
        (render_stored_order), written on the device in one engine call
        (RepoUJSON.get_resp, jy_ujson_get_resp).  The queries the device leaves
        to the host (a leaf too deep, a key to escape) are rendered here from
        one path read, by the same rule: the result does not depend on which
        side rendered.  Needs the device leaf store (DeviceLeaves)."""
        keys, paths = list(keys), [tuple(p) for p in paths]
        if not keys:
            return []
        if not self._device_paths():
            raise RuntimeError("get_resp needs documents and leaves on one engine (GpuDocs + DeviceLeaves)")
        with self.leaves.lock():
            rb, ro, on_host = self.b.r.get_resp(keys, paths)
        ro = [int(x) for x in ro]
        out = [rb[ro[i]:ro[i + 1]] for i in range(len(keys))]
        mine = [i for i in range(len(keys)) if on_host[i]]
        if mine:
            found = self.leaves.under(self.b.r.slots_of([keys[i] for i in mine]), [paths[i] for i in mine], leaves=True)
            for i, q in zip(mine, found):
                text = render_stored_order([leaf for _, leaf in q]).encode()
                out[i] = b"$%d\r\n%s\r\n" % (len(text), text)
        return out

    def ins(self, key, path, value):
        """INS (repo_ujson.pony:90-99)"""
        self.b.write([("INS", key, self.leaves.handle(path, canonical_value(value)))], self.identity)
        self._written()

    def rm(self, key, path, value):
        """RM (repo_ujson.pony:101-110): no key creation"""
        self.b.write([("RM", key, self.leaves.handle(path, canonical_value(value)))], self.identity)
        self._written()

    def clr(self, key, path=()):
        """CLR (repo_ujson.pony:85-88): no key creation; path-scoped"""
        if not self.b.exists(key):
            return
        if not path:
            self.b.write([("CLR", key)], self.identity)
            self._written()
            return
        hs = sorted(self._under(key, path))
        # nothing under the path still creates the key's delta (_delta_for)
        self.b.write([("RM", key, h) for h in hs] or [("TOUCH", key)], self.identity)
        self._written()

    def set(self, key, path, text):
        """SET (repo_ujson.pony:74-83): clear the path, then insert the node's leaves"""
        leaves = flatten(text, path)
        cmds = []
        if self.b.exists(key):
            if not path:
                cmds.append(("CLR", key))
            else:
                cmds += [("RM", key, h) for h in sorted(self._under(key, path))]
        cmds += [("INS", key, self.leaves.handle(p, v)) for p, v in sorted(leaves)]
        # an empty node still creates the key and its delta (_data_for, _delta_for)
        self.b.write(cmds or [("TOUCH", key)], self.identity)
        self._written()


    def apply(self, words):
        """one UJSON command as its RESP words (bytes or str; word 0 is UJSON) ->
        its reply bytes: GET key [path...] through get_resp, SET / INS / RM key
        [path...] value and CLR key [path...] -> +OK.  Any other op, or a
        command too short for its op, raises ValueError.
        This layer's documents are text: a key, segment or value that is not
        UTF-8 cannot be written through it (ValueError).  A GET is binary-safe
        as far as the device renders it -- such a key or segment is passed on as
        bytes and matches what a peer may have written; only where the render
        leaves that query to the host does it fail (UnicodeDecodeError), the
        leaves being decoded here."""
        def text(x):
            if not isinstance(x, (bytes, bytearray)):
                return str(x)
            try:
                return bytes(x).decode()
            except UnicodeDecodeError:
                return bytes(x)
        w = [text(x) for x in words]
        if len(w) < 3 or w[0] != "UJSON":
            raise ValueError("not a UJSON command: %r" % (w[:3],))
        op, key, rest = w[1], w[2], w[3:]
        if op == "GET":
            return self.get_resp([key], [tuple(rest)])[0]
        if any(isinstance(x, bytes) for x in w):
            raise ValueError("UJSON %s: a word is not UTF-8" % (op,))
        if op == "CLR":
            self.clr(key, tuple(rest))
            return b"+OK\r\n"
        if op not in ("SET", "INS", "RM"):
            raise ValueError("UJSON has no op %r" % (op,))
        if not rest:
            raise ValueError("UJSON %s needs a value" % op)
        {"SET": self.set, "INS": self.ins, "RM": self.rm}[op](key, tuple(rest[:-1]), rest[-1])
        return b"+OK\r\n"

    def resp_exec(self, conns, identity, on_host=None, device=False, ujson_write=False):
        """Engine.resp_exec(ujson_get=True) for a process whose UJSON repo is
        this object: UJSON GET is decoded and rendered on the device, every other
        UJSON command -- and a GET the render leaves to the host -- is answered
        by apply(), everything else no keyed call exists for by on_host(words).
        The repo's queued converges are drained first and the leaf store's lock
        is held for the whole call; apply's own engine calls, made from the
        callback on this thread, enter it again without taking it twice
        (DeviceLeaves.lock).  -> as Engine.resp_exec.
        ujson_write=True: UJSON INS / RM with a plain value (one that already is
        its canonical text) and UJSON CLR key are applied on the device too
        (jy_ujson_write_keys), under the same lock; SET, a CLR with a path and
        any other value still come to apply().  That path is binary-safe: the
        text-only restriction is apply()'s."""
        if not self._device_paths():
            raise RuntimeError("resp_exec needs documents and leaves on one engine (GpuDocs + DeviceLeaves)")
        self.b.r._drain()

        def answer(words):
            if words and bytes(words[0]) == b"UJSON":
                return self.apply(words)
            if on_host is None:
                raise ValueError("a command for the host and no on_host: %r" % (words[:2],))
            return on_host(words)

        with self.leaves.lock():
            out = self.b.r.eng.resp_exec(conns, identity, answer, device=device, ujson_get=True,
                                         ujson_write=ujson_write)
        if ujson_write:
            self._written()
        return out


class GpuDocs:
    """backend adapter: the GPU RepoUJSON"""

    def __init__(self, repo):
        self.r = repo

    def write(self, cmds, identity):
        self.r.write(cmds, identity)

    def exists(self, key):
        from . import engine as E
        return int(self.r.slots_of([key])[0]) != E._lib.JY_NO_SLOT

    def elements(self, keys):
        from . import engine as E
        slots = self.r.slots_of(keys)
        live = [(k, int(s)) for k, s in zip(keys, slots) if int(s) != E._lib.JY_NO_SLOT]
        if not live:
            return {}
        eo, dots, elems, vv, co, cloud = self.r.eng.ujson_read(np.array([s for _, s in live], np.uint32))
        return {k: elems[int(eo[i]):int(eo[i + 1])].tolist() for i, (k, _) in enumerate(live)}
