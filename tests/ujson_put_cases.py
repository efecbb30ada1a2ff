"""UJSON INS / RM / CLR as a keyed kind of the RESP decoder (JY_RESP_UJSON_WRITE)
and as a keyed write (jy_ujson_write_keys): the value rule, the classification
and the leaf encoding restated in Python, and the cases
tests/test_ujson_put_cpu.py and tests/test_ujson_put_gpu.py share.

value_plain is jy_resp_in.hpp's ujson_value_plain; classify is classify_opts +
classify_all under any flags (resp_ujson_cases.classify_lens stays the reference
of everything the write flag does not touch); decode is resp_in_ref.decode under
`flags`, a write row's value being ujson_doc._encode's bytes."""
import random
import re

import numpy as np

import resp_in_ref as ref
import resp_ujson_cases as UC
from resp_in_ref import request as R

UJSON_WRITE = 11
FLAG_GET, FLAG_WRITE = 1, 2
INS, RM, CLR = 0, 1, 2
VALUE_MAX = 255
WORDS_READ = UC.WORDS_READ
MAX = ref.MAX_KEYED
TERM = b"\xff\xff\xff\xff"

_PLAIN = re.compile(rb'\A(?:true|false|null|-?(?:0|[1-9][0-9]{0,17})|"[\x20\x21\x23-\x5b\x5d-\x7e]*")\Z')


def value_plain(w):
    """the word already is the canonical text of a JSON primitive the device may copy"""
    w = bytes(w)
    return len(w) <= VALUE_MAX and w != b"-0" and _PLAIN.match(w) is not None


def encode_leaf(segments, value):
    return UC.encode_path(segments) + TERM + bytes(value)


def classify(head, lens, flags, last=None):
    """head: the bytes of the first words, lens: the length of EVERY word, last:
    the bytes of the last word (None: unknown) -> (kind, op, num, key index,
    value index or None)"""
    n = len(lens)
    h = [bytes(x) for x in head]
    is_get = n >= 2 and len(h) >= 2 and h[1] == b"GET"
    if flags & FLAG_WRITE and n >= 1 and h and h[0] == b"UJSON" and not (flags & FLAG_GET and is_get):
        host = (ref.HOST, 0, 0, None, None)
        if n < 3 or lens[2] > MAX:
            return host
        op = h[1]
        if op == b"CLR":
            return (UJSON_WRITE, CLR, 0, 2, None) if n == 3 else host
        if op not in (b"INS", b"RM") or n < 4:
            return host
        if any(x > MAX for x in lens[3:n - 1]):
            return host
        if last is None or len(last) != lens[-1] or not value_plain(last):
            return host
        if sum(4 + x for x in lens[3:]) > MAX:
            return host
        return (UJSON_WRITE, INS if op == b"INS" else RM, 0, 2, None)
    return UC.classify_lens(h, lens, flags & FLAG_GET)


def classify_words(words, flags):
    words = [bytes(w) for w in words]
    return classify(words[:WORDS_READ], [len(w) for w in words], flags, words[-1] if words else None)


def decode(buf, conn_offs, flags):
    """resp_in_ref.decode under `flags` (resp_ujson_cases.decode with the write kind)"""
    buf = bytes(buf)
    nconn = len(conn_offs) - 1
    used, err = np.zeros(nconn, np.uint64), np.zeros(nconn, np.uint8)
    cmd_conn, cmd_kind, cmd_phase, cwo, woff, wlen = [], [], [], [0], [], []
    rows = []  # (phase, kind, command, key bytes, value bytes, num, op)
    for c in range(nconn):
        cmds, used[c], err[c] = ref.frame(buf, int(conn_offs[c]), int(conn_offs[c + 1]))
        phase, prev = 0, None
        for words in cmds:
            ws = [buf[o:o + n] for o, n in words]
            kind, op, num, ki, vi = classify_words(ws, flags)
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
            if kind == UC.UJSON_GET:
                value = UC.encode_path(ws[3:])
            elif kind == UJSON_WRITE:
                value = b"" if op == CLR else encode_leaf(ws[3:-1], ws[-1])
            else:
                value = b"" if vi is None else ws[vi]
            if kind != ref.HOST:
                rows.append((phase, kind, k, ws[ki], value, num, op))
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


# ---- the value rule's words ----
PRINTABLE = b'"' + bytes(c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C)) + b'"'
ACCEPTED = [b"0", b"-1", b"9" * 18, b'""', PRINTABLE, b'"' + b"x" * 253 + b'"', b"true", b"false", b"null",
            b"-" + b"9" * 18, b"10", b'" "']
REJECTED = [b"-0", b"01", b"1.0", b"1e3", b" 1", b"1 ", b"9" * 19, b'"a\\"b"', b'"', b"tru", b"", b'"a\x7fb"',
            b'"' + b"x" * 254 + b'"', b"-", b"+1", b"True", b"nul", b"nulll", b'"a"b"', b'"a', b'a"', b'"\xc3\xa9"',
            b'"a\nb"', b"1" * 256, b"--1", b"-01", b"[1]", b"{}"]
ALPHABET = b'"\\-+0123456789.e \x7f\n'


def random_words(seed, count, max_len=12):
    """seeded strings over quotes, backslashes, signs, digits, '.', 'e', blanks, DEL and newline"""
    rng = random.Random(seed)
    return [bytes(rng.choice(ALPHABET) for _ in range(rng.randrange(max_len + 1))) for _ in range(count)]


# ---- the rule's cases: (name, every word or None for a word that is a length alone, lens, flags) ----
VALUE_AT = (3, 4, 5, 9)  # the value's word index: inside the words a command lane reads, and beyond


def rule_cases():
    import resp_in_cases as RC
    out = []
    bufs, _ = RC.kinds(with_big=False)
    for i, b in enumerate(bufs):
        (words,) = ref.frame(b, 0, len(b))[0]
        ws = [b[o:o + n] for o, n in words]
        for flags in (0, 1, 2, 3):
            out.append(("kinds%d/%d" % (i, flags), ws, [len(w) for w in ws], flags))

    def uj(name, *words, lens=None, flags=FLAG_WRITE):
        ws = [w.encode() if isinstance(w, str) else w for w in words]
        out.append((name, ws, lens if lens is not None else [len(w) for w in ws], flags))

    values = ACCEPTED + REJECTED + random_words(7, 40)
    for at in VALUE_AT:
        segs = ["s%d" % j for j in range(at - 3)]
        for vi, v in enumerate(values):
            for op in ("INS", "RM"):
                uj("%s-at%d-v%d" % (op, at, vi), "UJSON", op, "k", *segs, v, flags=2 + (vi & 1))
    for flags in (0, 1):
        for op in ("INS", "RM", "CLR", "SET", "GET"):
            uj("off-%s/%d" % (op, flags), "UJSON", op, "k", *(["a", "1"] if op not in ("CLR", "GET") else []), flags=flags)
    uj("clr", "UJSON", "CLR", "k")
    uj("clr-path", "UJSON", "CLR", "k", "a")
    uj("clr-2-words", "UJSON", "CLR")
    uj("set", "UJSON", "SET", "k", "a", "1")
    uj("ins-3-words", "UJSON", "INS", "k")
    uj("ins-lower", "UJSON", "ins", "k", "1")
    uj("get-write-only", "UJSON", "GET", "k", "a")
    uj("get-both", "UJSON", "GET", "k", "a", flags=3)
    uj("key-max", "UJSON", "INS", None, b"1", lens=[5, 3, MAX, 1])
    uj("key-over", "UJSON", "INS", None, b"1", lens=[5, 3, MAX + 1, 1])
    # a segment over the limit at word 3 and at word 7; the leaf's total on both sides of the limit
    uj("seg3-over", "UJSON", "INS", "k", None, b"1", lens=[5, 3, 1, MAX + 1, 1])
    uj("seg7-over", "UJSON", "RM", "k", "a", "b", "c", "d", None, b"1", lens=[5, 2, 1, 1, 1, 1, 1, MAX + 1, 1])
    uj("leaf-max", "UJSON", "INS", "k", None, b"1", lens=[5, 3, 1, MAX - 9, 1])
    uj("leaf-over", "UJSON", "INS", "k", None, b"1", lens=[5, 3, 1, MAX - 8, 1])
    uj("leaf7-max", "UJSON", "INS", "k", "a", "b", "c", "d", None, b"1", lens=[5, 3, 1, 1, 1, 1, 1, MAX - 29, 1])
    uj("leaf7-over", "UJSON", "INS", "k", "a", "b", "c", "d", None, b"1", lens=[5, 3, 1, 1, 1, 1, 1, MAX - 28, 1])
    return out


def case_classify(words, lens, flags):
    head = [w if w is not None else b"" for w in words[:WORDS_READ]]
    return classify(head, lens, flags, words[-1] if words else None)


# ---- decoder inputs ----
PATH_WORDS = (0, 1, 4, 65)
BINARY = (b"\r\n", b"\0", b"\xff", b"$3\r\n", b"*1\r\n", b"\xff\xff\xff\xff")


def ins(key, *rest):
    return R("UJSON", "INS", key, *rest)


def rm(key, *rest):
    return R("UJSON", "RM", key, *rest)


def clr(key, *rest):
    return R("UJSON", "CLR", key, *rest)


def path_word_counts():
    """one connection per path length; INS and RM, the value beyond the words read"""
    out = []
    for n in PATH_WORDS:
        segs = [("s%d" % j) * (j % 4) for j in range(n)]
        out.append(ins("doc%d" % n, *segs, '"v%d"' % n) + rm("doc%d" % n, *segs, str(n)) + clr("doc%d" % n))
    return out


def value_lengths():
    """value lengths 1 to 17 behind 0 and 1 segments: leaf lengths on both sides of
    every multiple of 8; a value of 255 bytes, and one of 256 (the host's)"""
    cmds = []
    for n in range(1, 18):
        v = "7" * n if n <= 2 else '"' + "x" * (n - 2) + '"'
        cmds += [ins("k", v), ins("k", "abc", v), rm("k", "a", "", v)]
    cmds += [ins("long", "p", '"' + "y" * 253 + '"'), ins("long", "p", '"' + "y" * 254 + '"')]
    return [b"".join(cmds)]


def binary_values():
    """framing bytes inside a (string) value, a segment and a key"""
    vals = ['"$3\r\n"'.replace("\r\n", "  "), '"*1 $2"', '"+OK"']
    conn = b"".join(ins(s, s, '"ok"') for s in BINARY) + b"".join(ins("fr", v) for v in vals)
    # a value holding CR LF is not plain (a byte below 0x20): the host's
    return [conn, ins("fr", b'"$3\r\n"') + rm("fr", *BINARY, b"null")]


def block_edge(kthreads=256):
    """about 300 commands, so that rows (and words) cross a workgroup's edge, other kinds between"""
    cmds = []
    for i in range(kthreads + 44):
        op = (ins, rm)[i % 3 == 1]
        cmds.append(op("d%d" % (i % 11), *["p%d" % j for j in range(i % 7)], str(i)) if i % 9 else clr("d%d" % (i % 11)))
        if i % 10 == 0:
            cmds.append(R("TREG", "SET", "r%d" % i, "value %d" % i, i))
        if i % 17 == 0:
            cmds.append(R("UJSON", "INS", "d1", "f", "1.5"))  # not plain
    return [b"".join(cmds[:len(cmds) // 2]), b"".join(cmds[len(cmds) // 2:])]


def phases():
    """UJSON INS | UJSON SET | UJSON GET on one connection is three phases"""
    a = [ins("d", "a", "1"), R("UJSON", "SET", "d", "a", "2"), UC.get("d", "a"), rm("d", "a", "2"), clr("d"),
         clr("d", "a"), ins("d", "b", "1.0")]
    return [b"".join(a), b"".join(reversed(a))]


def cuts():
    """a command cut inside its value word, and a malformed token where the value stands"""
    whole = ins("k", "first", '"v"')
    tail = ins("k", "alpha", '"value"')
    inside = tail[:tail.index(b'"value"') + 3]
    bad = whole + tail[:tail.index(b"$7\r\n")] + b"$x\r\n" + whole
    return [(whole + inside, len(whole), False), (bad, len(whole), True)]


def all_inputs():
    return (path_word_counts() + value_lengths() + binary_values() + block_edge() + phases() +
            [b for b, _, _ in cuts()] + UC.with_ujson_commands())
