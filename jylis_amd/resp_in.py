"""Bytes in, bytes out: the receive buffers of a heartbeat's connections decoded
on the GPU (Engine.resp_decode), applied as one keyed call per group and
answered as RESP reply bytes.

The decoder leaves its columns in HBM; the host only walks the small group
table in phase order.  A write group answers +OK, a read group goes through
Engine.*_get_resp, and the commands no keyed call exists for (kind CMD_HOST:
UJSON, SYSTEM, anything malformed as a command) are handed to `on_host` with
the words the decoder already cut.  jy_tlog_get_resp takes `what` and `count`
from host memory, so a TLOG read group downloads those two small columns.
Engine.resp_exec does all of this in one engine call; this loop is its reference.

With ujson_get=True `UJSON GET` is a keyed kind too (CMD_UJSON_GET): its group
is one Engine.ujson_get_resp call, the paths cut from the decoded value column,
and the queries that call leaves to the host go to `on_host` with the phase's
HOST commands, in command order.

With ujson_write=True `UJSON INS / RM` with a plain value and `UJSON CLR key` are
a keyed kind as well (CMD_UJSON_WRITE): its group is one
Engine.ujson_write_keys call with the decoded op, key and value (leaf) columns.
"""
import numpy as np

from . import _lib
from ._lib import GCOUNT, PNCOUNT

OK = b"+OK\r\n"

# kind -> (counter type, sign) of the counter writes
_COUNTER_WRITES = {_lib.CMD_GCOUNT_INC: (GCOUNT, 0), _lib.CMD_PNCOUNT_INC: (PNCOUNT, 0),
                   _lib.CMD_PNCOUNT_DEC: (PNCOUNT, 1)}
_COUNTER_READS = {_lib.CMD_GCOUNT_GET: GCOUNT, _lib.CMD_PNCOUNT_GET: PNCOUNT}


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _cut(reply):
    rb, ro = bytes(_host(reply["reply_bytes"]).tobytes()), _host(reply["reply_offs"]).astype(np.int64)
    return [rb[ro[i]:ro[i + 1]] for i in range(len(ro) - 1)]


def _paths(vb, vo):
    """the value column of a CMD_UJSON_GET group -> one tuple of segments (bytes) per row"""
    out = []
    for a, b in zip(vo[:-1], vo[1:]):
        path, at = [], int(a)
        while at < int(b):
            n = int.from_bytes(vb[at:at + 4], "little")
            path.append(vb[at + 4:at + 4 + n])
            at += 4 + n
        assert at == int(b)
        out.append(tuple(path))
    return out


def run_group(engine, d, g, col, identity=None):
    """the keyed call of group g of a decode `d` (device columns, untouched) ->
    the group's replies in row order (None: a UJSON GET left to the host)"""
    a, b = int(d["group_offs"][g]), int(d["group_offs"][g + 1])
    kind = int(d["group_class"][g])
    keys = (d["key_bytes"], d["key_offs"][a:b + 1])
    num = d["num"][a:b]
    if kind in _COUNTER_WRITES:
        ctype, sign = _COUNTER_WRITES[kind]
        engine.counter_write_keys(ctype, sign, col, keys, num)
        return [OK] * (b - a)
    if kind == _lib.CMD_TREG_SET:
        engine.treg_set_keys(keys, num, (d["val_bytes"], d["val_offs"][a:b + 1]))
        return [OK] * (b - a)
    if kind == _lib.CMD_TLOG_WRITE:
        engine.tlog_write_keys(d["op"][a:b], keys, ts=num, arg=num, values=(d["val_bytes"], d["val_offs"][a:b + 1]))
        return [OK] * (b - a)
    if kind in _COUNTER_READS:
        return _cut(engine.counter_get_resp(_COUNTER_READS[kind], keys))
    if kind == _lib.CMD_TREG_GET:
        return _cut(engine.treg_get_resp(keys))
    if kind == _lib.CMD_TLOG_READ:
        count = _host(num).view(np.uint64)
        return _cut(engine.tlog_get_resp(keys, count=count, what=_host(d["op"][a:b])))
    if kind == _lib.CMD_UJSON_GET:
        vb, vo = bytes(_host(d["val_bytes"]).tobytes()), _host(d["val_offs"][a:b + 1]).astype(np.int64)
        r = engine.ujson_get_resp(keys, _paths(vb, vo))
        return [None if h else x for x, h in zip(_cut(r), _host(r["on_host"]))]
    if kind == _lib.CMD_UJSON_WRITE:
        engine.ujson_write_keys(d["op"][a:b], keys, (d["val_bytes"], d["val_offs"][a:b + 1]), identity)
        return [OK] * (b - a)
    raise ValueError(f"group {g} has kind {kind}")


def exec_resp(engine, conn_buffers, identity, on_host, ujson_get=False, ujson_write=False):
    """Decode the connections' receive buffers, apply their commands and answer
    them.  conn_buffers: a list of bytes, one per connection, each starting at
    a command boundary.  identity: this replica's id (its column takes the
    counter writes).  on_host(words) -> the reply bytes of a command no keyed
    call exists for.
    -> one (reply bytes, bytes consumed, closed) per connection: the replies of
    its complete commands in command order, how many of its bytes they took
    (the caller keeps the rest), and whether what follows is malformed.
    ujson_get=True: UJSON GET is decoded and rendered on the device; on_host
    also answers the GETs the render leaves to the host (the caller holds the
    leaf store's lock).
    ujson_write=True: UJSON INS / RM / CLR are decoded on the device and applied
    with one Engine.ujson_write_keys per group (the same lock)."""
    bufs = [bytes(b) for b in conn_buffers]
    req = b"".join(bufs)
    offs = np.zeros(len(bufs) + 1, np.uint64)
    if bufs:
        offs[1:] = np.cumsum([len(b) for b in bufs], dtype=np.uint64)
    d = engine.resp_decode((req, offs), device=True, ujson_get=ujson_get, ujson_write=ujson_write)
    engine.sync()
    ncmd = d["sizes"][0]
    cmd_conn, cmd_kind, cmd_phase = (_host(d[k]) for k in ("cmd_conn", "cmd_kind", "cmd_phase"))
    replies = [None] * ncmd
    hosts = np.flatnonzero(cmd_kind == _lib.CMD_HOST)
    if len(hosts) or ujson_get:
        cwo, woff, wlen = (_host(d[k]).astype(np.int64) for k in ("cmd_word_offs", "word_off", "word_len"))
    col = engine.replica_col(identity)
    row_cmd = _host(d["row_cmd"])
    ngroups, g, h = d["sizes"][5], 0, 0
    nphases = int(cmd_phase.max()) + 1 if ncmd else 0
    host_order = hosts[np.argsort(cmd_phase[hosts], kind="stable")]
    for phase in range(nphases):
        mine = []  # this phase's commands for on_host
        while g < ngroups and int(d["group_phase"][g]) == phase:
            a = int(d["group_offs"][g])
            for j, r in enumerate(run_group(engine, d, g, col, identity)):
                replies[int(row_cmd[a + j])] = r
                if r is None:
                    mine.append(int(row_cmd[a + j]))
            g += 1
        while h < len(host_order) and cmd_phase[host_order[h]] == phase:
            mine.append(int(host_order[h]))
            h += 1
        for k in sorted(mine):
            replies[k] = on_host([req[woff[w]:woff[w] + wlen[w]] for w in range(cwo[k], cwo[k + 1])])
    out = [[] for _ in bufs]
    for k in range(ncmd):
        out[int(cmd_conn[k])].append(replies[k])
    used, err = _host(d["conn_used"]), _host(d["conn_err"])
    return [(b"".join(out[c]), int(used[c]), bool(err[c])) for c in range(len(bufs))]
