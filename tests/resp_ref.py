"""Reference of the RESP replies (jy_*_get_resp) in pure Python.

Input: the answers of tests/get_ref.py (themselves built from an oracle
Repo.state() table).  Output: the reply bytes and offsets the calls return, as
jemc/pony-resp's Respond writes them (the table in include/jylis_gpu.h):
numbers in decimal, no leading zeros, no '+'.  Shares no code with the product.

Every function returns (bytes, offs, pieces): reply i is
bytes[offs[i]:offs[i + 1]]; pieces lists the stream's pieces in order as
(kind, byte string) with kind "qhead" | "ehead" | "value" | "etail" -- what
the case-table conditions of tests/test_get_resp_cpu.py are stated on.
"""
import numpy as np

import get_ref

GET, SIZE, CUTOFF = 0, 1, 2
CRLF = b"\r\n"


def _num(v):
    return str(int(v)).encode()


def _entry(value, ts):
    return [("ehead", b"*2" + CRLF + b"$" + _num(len(value)) + CRLF), ("value", bytes(value)),
            ("etail", CRLF + b":" + _num(ts) + CRLF)]


def _finish(per_query):
    """per query its pieces -> (bytes, offs u64[n + 1], all pieces)"""
    offs, out, pieces = [0], [], []
    for ps in per_query:
        out.append(b"".join(b for _, b in ps))
        offs.append(offs[-1] + len(out[-1]))
        pieces += ps
    return b"".join(out), np.array(offs, np.uint64), pieces


def treg(ans):
    """a get_ref.treg_get answer -> replies; sizes = [reply bytes, keys found]"""
    per = []
    for q in range(len(ans["found"])):
        r = get_ref.treg_reply(ans, q)
        per.append([("qhead", b"$-1" + CRLF)] if r is None else _entry(*r))
    return _finish(per)


def tlog(ans, what=None):
    """a get_ref.tlog_get answer (computed with the counts) -> replies.  what:
    None (GET throughout) or GET / SIZE / CUTOFF per query; SIZE and CUTOFF
    answer whatever the count was and list no entry"""
    per = []
    for q in range(len(ans["found"])):
        w = GET if what is None else int(what[q])
        if w == SIZE:
            per.append([("qhead", b":" + _num(ans["size"][q]) + CRLF)])
        elif w == CUTOFF:
            per.append([("qhead", b":" + _num(ans["cutoff"][q]) + CRLF)])
        else:
            ents = get_ref.tlog_reply(ans, q)
            ps = [("qhead", b"*" + _num(len(ents)) + CRLF)]
            for v, ts in ents:
                ps += _entry(v, ts)
            per.append(ps)
    return _finish(per)


def tlog_entries(ans, what=None):
    """entries the replies list (sizes_out[1])"""
    eo = ans["ent_offs"].astype(np.int64)
    return int(sum(int(eo[q + 1] - eo[q]) for q in range(len(eo) - 1) if what is None or int(what[q]) == GET))


def from_treg(replies):
    """per key what TREG GET returns -- (value, ts), or None -- -> replies"""
    return _finish([[("qhead", b"$-1" + CRLF)] if r is None else _entry(*r) for r in replies])


def from_tlog(replies):
    """per key what TLOG GET returns -- [(value, ts)] -- -> replies"""
    return _finish([[("qhead", b"*" + _num(len(es)) + CRLF)] + [p for v, ts in es for p in _entry(v, ts)]
                    for es in replies])


def counter(values):
    """the values of get_ref.counter_get (uint64 for GCOUNT, int64 for PNCOUNT) -> replies"""
    return _finish([[("qhead", b":" + _num(v) + CRLF)] for v in values])


def split(rb, ro):
    """(bytes, offs) -> the list of replies"""
    rb = bytes(rb)
    return [rb[int(ro[i]):int(ro[i + 1])] for i in range(len(ro) - 1)]
