"""UJSON GET as a keyed kind of the RESP decoder (JY_RESP_UJSON_GET): the rule
and the path encoding restated in Python next to tests/resp_in_ref.py, which
stays the reference of everything else, and the cases tests/test_resp_ujson_cpu.py
and tests/test_resp_ujson_gpu.py share.

classify_opts(words, flags) is jy_resp_in.hpp's classify_opts + classify_all;
decode(buf, conn_offs, flags) is resp_in_ref.decode with that rule, a UJSON GET
row's value being encode_path(its words from 3 on)."""
import numpy as np

import resp_in_ref as ref
from resp_in_ref import request as R

UJSON_GET = 10
FLAG = 1          # JY_RESP_UJSON_GET
WORDS_READ = 5    # jyrin::kWordsRead
MAX = ref.MAX_KEYED


def encode_path(segments):
    """per segment the 4-byte little-endian length, then the bytes; no terminator"""
    return b"".join(len(s).to_bytes(4, "little") + bytes(s) for s in segments)


def classify_lens(head, lens, flags):
    """head: the bytes of the first words (at least the type and the op where
    there are that many), lens: the length of EVERY word -> (kind, op, num, key
    index, value index or None).  Only lengths are looked at past the op."""
    n = len(lens)
    if flags & FLAG and n >= 1 and bytes(head[0]) == b"UJSON":
        host = (ref.HOST, 0, 0, None, None)
        if n < 3 or lens[2] > MAX or bytes(head[1]) != b"GET":
            return host
        if any(x > MAX for x in lens[3:]):
            return host
        return (UJSON_GET, 0, 0, 2, None)
    # every other type reads only words of `head`, which hold their bytes (UJSON without the flag reads none)
    return ref.classify([bytes(head[j]) if j < len(head) else b"" for j in range(n)])


def classify_opts(words, flags):
    return classify_lens(words[:WORDS_READ], [len(w) for w in words], flags)


def decode(buf, conn_offs, flags):
    """resp_in_ref.decode under `flags`"""
    buf = bytes(buf)
    nconn = len(conn_offs) - 1
    used, err = np.zeros(nconn, np.uint64), np.zeros(nconn, np.uint8)
    cmd_conn, cmd_kind, cmd_phase, cwo, woff, wlen = [], [], [], [0], [], []
    rows = []  # (phase, kind, command, key bytes, value bytes, num, op)
    for c in range(nconn):
        cmds, used[c], err[c] = ref.frame(buf, int(conn_offs[c]), int(conn_offs[c + 1]))
        phase, prev = 0, None
        for words in cmds:
            head = [buf[o:o + n] for o, n in words[:WORDS_READ]]
            kind, op, num, ki, vi = classify_lens(head, [n for _, n in words], flags)
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
            if kind == UJSON_GET:
                value = encode_path([buf[o:o + n] for o, n in words[3:]])
            else:
                value = b"" if vi is None else buf[words[vi][0]:words[vi][0] + words[vi][1]]
            if kind != ref.HOST:
                o, n = words[ki]
                rows.append((phase, kind, k, buf[o:o + n], value, num, op))
    rows.sort(key=lambda r: (r[0], r[1]))
    keys, vals = [r[3] for r in rows], [r[4] for r in rows]
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


# ---- the rule's cases: (name, head words, every word's length, flags) ----
def rule_cases():
    import resp_in_cases as RC
    out = []
    # flags off (and on): every existing case classifies as classify does
    bufs, _ = RC.kinds(with_big=False)
    for i, b in enumerate(bufs):
        (words,) = ref.frame(b, 0, len(b))[0]
        ws = [b[o:o + n] for o, n in words]
        for flags in (0, FLAG):
            out.append(("kinds%d/%d" % (i, flags), ws[:WORDS_READ], [len(w) for w in ws], flags))

    def uj(name, *words, lens=None, flags=FLAG):
        ws = [w.encode() for w in words]
        out.append((name, ws[:2], lens if lens is not None else [len(w) for w in ws], flags))

    uj("get-off", "UJSON", "GET", "k", flags=0)
    uj("get-2-words", "UJSON", "GET")
    uj("get-whole", "UJSON", "GET", "k")
    uj("get-path", "UJSON", "GET", "k", "a", "b")
    uj("get-lower-op", "UJSON", "get", "k")
    uj("get-lower-type", "ujson", "GET", "k")
    for op in ("SET", "CLR", "INS", "RM"):
        uj("write-" + op, "UJSON", op, "k", "a", "1")
    uj("key-max", "UJSON", "GET", "k", lens=[5, 3, MAX])
    uj("key-over", "UJSON", "GET", "k", lens=[5, 3, MAX + 1])
    for at in (3, 7):  # word 7 lies beyond the words a command lane reads
        for n in (MAX, MAX + 1):
            lens = [5, 3, 1] + [2] * (at - 3) + [n] + [1]
            uj("seg%d-%s" % (at, "max" if n == MAX else "over"), "UJSON", "GET", "k", lens=lens)
    return out


# ---- decoder inputs ----
PATH_WORDS = (0, 1, 2, 5, 6, 63, 64, 65)   # the edges of kWordsRead (5 words = 2 segments) and of a wave
SEG_LENS = (0, 1, 7, 8, 9, 255)            # the 8-byte load steps
BINARY = (b"\r\n", b"\0", b"\xff", b"$3\r\n", b"*1\r\n", b"a\r\n$1\r\nb", b"\xff\xff\xff\xff")


def get(key, *segments):
    return R("UJSON", "GET", key, *segments)


def path_word_counts():
    """one connection per path length, segments of differing lengths"""
    return [get("doc%d" % n, *[("s%d" % j) * (j % 4) for j in range(n)]) for n in PATH_WORDS]


def segment_lengths():
    return [b"".join(get("k", bytes([65 + i]) * n, b"x" * n) for i, n in enumerate(SEG_LENS))]


def binary_segments():
    return [get("bin", *BINARY), b"".join(get(s, s) for s in BINARY)]


def block_edge(kthreads=256):
    """enough commands that path words (and tokens) cross a workgroup's edge, with
    other kinds in between"""
    cmds = []
    for i in range(kthreads // 2 + 20):
        cmds.append(get("d%d" % (i % 7), *["p%d" % j for j in range(i % 6)]))
        if i % 5 == 0:
            cmds.append(R("TREG", "SET", "r%d" % i, "value %d" % i, i))
    return [b"".join(cmds[:len(cmds) // 2]), b"".join(cmds[len(cmds) // 2:])]


def phases():
    a = [R("UJSON", "SET", "d", "a", "1"), get("d", "a"), get("d"), R("TREG", "GET", "t"), get("d", "b", "c")]
    b = [a[3], a[1], a[0], a[4], a[2]]
    return [b"".join(a), b"".join(b)]


def cuts():
    """a command cut inside a path word, inside a path word's header, and a
    malformed token inside a path: (buffer, bytes used, closed)"""
    whole = get("k", "first")
    tail = get("k", "alpha", "beta")
    inside = tail[:tail.index(b"alpha") + 3]
    header = tail[:tail.index(b"$5\r\nalpha") + 2]
    bad = whole + R("UJSON", "GET", "k", "alpha")[:-len(b"$5\r\nalpha\r\n")] + b"$x\r\nalpha\r\n" + whole
    return [(whole + inside, len(whole), False), (whole + header, len(whole), False), (bad, len(whole), True)]


def with_ujson_commands():
    """an input that holds UJSON commands, for the flags-0 comparison"""
    return phases() + binary_segments() + [R("UJSON", "INS", "d", "tags", '"x"') + get("d", "tags") + R("GCOUNT", "GET", "g")]
