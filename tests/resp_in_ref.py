"""A plain sequential decoder of RESP requests: the contract of jy_resp_decode
(include/jylis_gpu.h "RESP requests") restated in Python, one connection and one
byte run at a time, with no knowledge of how the GPU decoder is built.

decode(buf, conn_offs) returns every array of the call as numpy arrays; the
GPU tests compare element for element.  request(*words) writes a command the
way a client does."""
import numpy as np

(HOST, GCOUNT_INC, GCOUNT_GET, PNCOUNT_INC, PNCOUNT_DEC, PNCOUNT_GET, TREG_SET, TREG_GET, TLOG_WRITE,
 TLOG_READ) = range(10)
TLOG_INS, TLOG_TRIMAT, TLOG_TRIM, TLOG_CLR = 0, 1, 2, 3
RD_GET, RD_SIZE, RD_CUTOFF = 0, 1, 2
ALL = 2**64 - 1
MAX_KEYED = 2**24 - 1

COMPLETE, INCOMPLETE, MALFORMED = 0, 1, 2


def _b(x):
    return x if isinstance(x, (bytes, bytearray)) else str(x).encode()


def request(*words):
    """the words of one command as a client sends them"""
    return b"*%d\r\n" % len(words) + b"".join(b"$%d\r\n%s\r\n" % (len(_b(w)), _b(w)) for w in words)


def _number(buf, pos, end):
    """the decimal after a token's first byte -> (status, value, position after \\r\\n)"""
    v, nd, i = 0, 0, pos
    while True:
        if i >= end:
            return INCOMPLETE, 0, 0
        c = buf[i]
        if 48 <= c <= 57:
            nd += 1
            v = v * 10 + (c - 48)
            if nd > 20 or v > ALL:
                return MALFORMED, 0, 0
            i += 1
            continue
        if c != 13 or nd == 0:
            return MALFORMED, 0, 0
        break
    if i + 1 >= end:
        return INCOMPLETE, 0, 0
    if buf[i + 1] != 10:
        return MALFORMED, 0, 0
    return COMPLETE, v, i + 2


def header_at(buf, pos, end):
    """-> (status, n, position after the header); the byte at pos is '*'"""
    return _number(buf, pos + 1, end)


def bulk_at(buf, pos, end):
    """-> (status, body, len, position after the string); the byte at pos is '$'"""
    st, n, body = _number(buf, pos + 1, end)
    if st != COMPLETE:
        return st, 0, 0, 0
    if body + n >= end:
        return INCOMPLETE, 0, 0, 0
    if buf[body + n] != 13:
        return MALFORMED, 0, 0, 0
    if body + n + 1 >= end:
        return INCOMPLETE, 0, 0, 0
    if buf[body + n + 1] != 10:
        return MALFORMED, 0, 0, 0
    return COMPLETE, body, n, body + n + 2


def parse_u64(s):
    if not 1 <= len(s) <= 20 or not all(48 <= c <= 57 for c in s):
        return None
    v = int(s)
    return v if v <= ALL else None


def parse_i64(s):
    if len(s) == 0:
        return None
    neg = s[:1] == b"-"
    m = parse_u64(s[1:] if neg or s[:1] == b"+" else s)
    if m is None or m > (2**63 if neg else 2**63 - 1):
        return None
    return -m if neg else m


def classify(words):
    """words: the command's byte strings -> (kind, op, num, key index, value index or None)"""
    host = (HOST, 0, 0, None, None)
    w = [bytes(x) for x in words[:5]]
    n = len(words)
    if n < 3 or len(words[2]) > MAX_KEYED:
        return host
    t, o = w[0], w[1]
    if t in (b"GCOUNT", b"PNCOUNT"):
        g = t == b"GCOUNT"
        if o == b"GET":
            return (GCOUNT_GET if g else PNCOUNT_GET, 0, 0, 2, None)
        if not (o == b"INC" or (o == b"DEC" and not g)) or n < 4:
            return host
        v = parse_u64(w[3]) if g else parse_i64(w[3])
        if v is None:
            return host
        kind = GCOUNT_INC if g else (PNCOUNT_INC if o == b"INC" else PNCOUNT_DEC)
        return (kind, 0, v % 2**64, 2, None)
    if t == b"TREG":
        if o == b"GET":
            return (TREG_GET, 0, 0, 2, None)
        if o != b"SET" or n < 5 or len(words[3]) > MAX_KEYED or parse_u64(w[4]) is None:
            return host
        return (TREG_SET, 0, parse_u64(w[4]), 2, 3)
    if t == b"TLOG":
        if o == b"GET":
            cnt = parse_u64(w[3]) if n >= 4 else None
            return (TLOG_READ, RD_GET, ALL if cnt is None else cnt, 2, None)
        if o in (b"SIZE", b"CUTOFF"):
            return (TLOG_READ, RD_SIZE if o == b"SIZE" else RD_CUTOFF, 0, 2, None)
        if o == b"INS":
            if n < 5 or len(words[3]) > MAX_KEYED or parse_u64(w[4]) is None:
                return host
            return (TLOG_WRITE, TLOG_INS, parse_u64(w[4]), 2, 3)
        if o in (b"TRIMAT", b"TRIM"):
            if n < 4 or parse_u64(w[3]) is None:
                return host
            return (TLOG_WRITE, TLOG_TRIM if o == b"TRIM" else TLOG_TRIMAT, parse_u64(w[3]), 2, None)
        if o == b"CLR":
            return (TLOG_WRITE, TLOG_CLR, 0, 2, None)
    return host


def frame(buf, start, end, toks=None):
    """one connection's bytes buf[start:end] -> ([(words as (off, len))], used, err);
    toks (a list) collects (position, first byte) of every complete token followed"""
    cmds, pos = [], start
    while True:
        used = pos - start
        if pos >= end:
            return cmds, used, 0
        if buf[pos] != 42:  # only '*' starts a command
            return cmds, used, 1
        st, n, p = header_at(buf, pos, end)
        if st != COMPLETE:
            return cmds, used, int(st == MALFORMED)
        if toks is not None:
            toks.append((pos, 42))
        words = []
        for _ in range(n):
            if p >= end:
                return cmds, used, 0
            if buf[p] != 36:  # only '$' starts a word
                return cmds, used, 1
            st, body, ln, q = bulk_at(buf, p, end)
            if st != COMPLETE:
                return cmds, used, int(st == MALFORMED)
            if toks is not None:
                toks.append((p, 36))
            words.append((body, ln))
            p = q
        cmds.append(words)
        pos = p


def decode(buf, conn_offs):
    buf = bytes(buf)
    nconn = len(conn_offs) - 1
    used, err = np.zeros(nconn, np.uint64), np.zeros(nconn, np.uint8)
    cmd_conn, cmd_kind, cmd_phase, cwo, woff, wlen = [], [], [], [0], [], []
    rows = []  # (phase, kind, command, key range, value range, num, op)
    for c in range(nconn):
        cmds, used[c], err[c] = frame(buf, int(conn_offs[c]), int(conn_offs[c + 1]))
        phase, prev = 0, None
        for words in cmds:
            kind, op, num, ki, vi = classify([buf[o:o + n] for o, n in words[:5]] + [b""] * max(0, len(words) - 5))
            if prev is not None and kind != prev:
                phase += 1
            prev = kind
            k = len(cmd_conn)
            cmd_conn.append(c)
            cmd_kind.append(kind)
            cmd_phase.append(phase)
            for o, n in words:
                woff.append(o)
                wlen.append(n)
            cwo.append(len(woff))
            if kind != HOST:
                rows.append((phase, kind, k, words[ki], words[vi] if vi is not None else (0, 0), num, op))
    rows.sort(key=lambda r: (r[0], r[1]))  # stable: stream order inside a group
    keys = [buf[o:o + n] for _, _, _, (o, n), _, _, _ in rows]
    vals = [buf[o:o + n] for _, _, _, _, (o, n), _, _ in rows]
    gph, gcl, goff = [], [], []
    for r, row in enumerate(rows):
        if r == 0 or row[:2] != rows[r - 1][:2]:
            gph.append(row[0])
            gcl.append(row[1])
            goff.append(r)
    goff.append(len(rows))
    cum = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs], dtype=np.uint64)]).astype(np.uint64)
    return {
        "conn_used": used, "conn_err": err,
        "cmd_conn": np.array(cmd_conn, np.uint32), "cmd_kind": np.array(cmd_kind, np.uint8),
        "cmd_phase": np.array(cmd_phase, np.uint32), "cmd_word_offs": np.array(cwo, np.uint64),
        "word_off": np.array(woff, np.uint64), "word_len": np.array(wlen, np.uint64),
        "row_cmd": np.array([r[2] for r in rows], np.uint32),
        "key_bytes": np.frombuffer(b"".join(keys), np.uint8), "key_offs": cum(keys),
        "val_bytes": np.frombuffer(b"".join(vals), np.uint8), "val_offs": cum(vals),
        "num": np.array([r[5] for r in rows], np.uint64), "op": np.array([r[6] for r in rows], np.uint8),
        "group_phase": np.array(gph, np.uint32), "group_class": np.array(gcl, np.uint8),
        "group_offs": np.array(goff, np.uint64),
        "sizes": [len(cmd_conn), len(woff), len(rows), sum(map(len, keys)), sum(map(len, vals)), len(gph)],
    }


def join(buffers):
    """connection buffers -> (bytes, conn_offs)"""
    offs = np.zeros(len(buffers) + 1, np.uint64)
    if buffers:
        offs[1:] = np.cumsum([len(b) for b in buffers], dtype=np.uint64)
    return b"".join(bytes(b) for b in buffers), offs


def commands(res, buf, c=None):
    """the decoded commands as word lists (of connection c, or all)"""
    out = []
    for k in range(len(res["cmd_conn"])):
        if c is not None and res["cmd_conn"][k] != c:
            continue
        a, b = int(res["cmd_word_offs"][k]), int(res["cmd_word_offs"][k + 1])
        out.append([bytes(buf[int(res["word_off"][w]):int(res["word_off"][w]) + int(res["word_len"][w])])
                    for w in range(a, b)])
    return out
