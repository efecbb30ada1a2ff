"""The request buffers tests/test_resp_in_cpu.py and tests/test_resp_in_gpu.py
share.  Every function returns a list of connection buffers (bytes); the CPU
file asserts what they cover, the GPU file decodes them and compares with
tests/resp_in_ref.py."""
from resp_in_ref import request as R

# ---- the two sweeps ----
# three commands, 117 bytes: a write with a value, a read with a count, a HOST command
_THREE = (R("TREG", "SET", "key1", "hello world", 10), R("TLOG", "GET", "chat", 2), R("SYSTEM", "GETLOG"))
THREE = b"".join(_THREE)
THREE_ENDS = (len(_THREE[0]), len(_THREE[0]) + len(_THREE[1]), len(THREE))  # 59, 99, 127: where its commands end
# two commands whose framing bytes the corruption sweep changes one at a time
TWO = R("TLOG", "INS", "k", "v\r\n", 7) + R("GCOUNT", "GET", "k")


def prefix_sweep():
    """every prefix of THREE, the whole included, a connection of its own"""
    return [THREE[:n] for n in range(len(THREE) + 1)]


def framing_positions(buf):
    """the positions of the bytes that are framing, not word content: headers,
    '$<len>\\r\\n' and the '\\r\\n' after every string"""
    import resp_in_ref as ref
    toks, content = [], set()
    cmds, used, err = ref.frame(buf, 0, len(buf), toks)
    assert used == len(buf) and err == 0
    for words in cmds:
        for o, n in words:
            content.update(range(o, o + n))
    return [i for i in range(len(buf)) if i not in content]


def corruption_sweep():
    """every framing byte of TWO replaced by each of 'x', '0', '9', '$', '*', '\\r',
    '\\n' that differs from it: one connection per corruption.  (A count or
    length raised to 9 leaves the connection waiting for bytes: not an error.)"""
    out = []
    for i in framing_positions(TWO):
        for c in b"x09$*\r\n":
            if TWO[i] != c:
                out.append(TWO[:i] + bytes([c]) + TWO[i + 1:])
    return out


# ---- every class and every HOST reason ----
BIG = 2**24 - 1  # the longest key or value a keyed call takes


def kinds(with_big=True):
    """one command per connection -> (buffers, expected kinds by name)"""
    rows = [
        ("GCOUNT_INC", R("GCOUNT", "INC", "g", 2**64 - 1)),
        ("GCOUNT_GET", R("GCOUNT", "GET", "g")),
        ("PNCOUNT_INC", R("PNCOUNT", "INC", "p", "+9223372036854775807")),
        ("PNCOUNT_INC", R("PNCOUNT", "INC", "p", "-9223372036854775808")),
        ("PNCOUNT_DEC", R("PNCOUNT", "DEC", "p", -5)),
        ("PNCOUNT_GET", R("PNCOUNT", "GET", "p")),
        ("TREG_SET", R("TREG", "SET", "r", "value", "00000000000000000012")),
        ("TREG_SET", R("TREG", "SET", "", "", 0)),  # an empty key and an empty value
        ("TREG_GET", R("TREG", "GET", "r")),
        ("TLOG_WRITE", R("TLOG", "INS", "l", "entry", 5)),
        ("TLOG_WRITE", R("TLOG", "TRIMAT", "l", 4)),
        ("TLOG_WRITE", R("TLOG", "TRIM", "l", 3)),
        ("TLOG_WRITE", R("TLOG", "CLR", "l")),
        ("TLOG_READ", R("TLOG", "GET", "l")),
        ("TLOG_READ", R("TLOG", "GET", "l", 7)),
        ("TLOG_READ", R("TLOG", "GET", "l", "many")),  # an unparsable count reads as all
        ("TLOG_READ", R("TLOG", "SIZE", "l")),
        ("TLOG_READ", R("TLOG", "CUTOFF", "l")),
        ("TREG_GET", R("TREG", "GET", "r", "ignored", "words", "beyond", "the", "key")),
        # HOST: no keyed call exists, or the command does not parse
        ("HOST", R("UJSON", "GET", "doc")),
        ("HOST", R("SYSTEM", "GETLOG")),
        ("HOST", R("NOPE", "GET", "k")),
        ("HOST", R("TREG", "NOPE", "k")),
        ("HOST", R("treg", "GET", "k")),
        ("HOST", R("TREG", "get", "k")),
        ("HOST", R("TREG", "SET", "k", "v")),  # a missing word
        ("HOST", R("TREG", "GET")),
        ("HOST", R("TREG")),
        ("HOST", R()),  # a command of no words
        ("HOST", R("TREG", "SET", "k", "v", "12x")),
        ("HOST", R("TREG", "SET", "k", "v", "18446744073709551616")),
        ("HOST", R("GCOUNT", "INC", "k", "-1")),
        ("HOST", R("GCOUNT", "DEC", "k", "1")),
        ("HOST", R("PNCOUNT", "INC", "k", "9223372036854775808")),
        ("HOST", R("PNCOUNT", "DEC", "k", "-9223372036854775809")),
        ("HOST", R("TLOG", "INS", "k", "v", "")),
        ("HOST", R("TLOG", "TRIM", "k", "x")),
        ("HOST", R("TLOG", "TRIMAT", "k")),
    ]
    if with_big:  # the 16 MiB rule, either side of it, for a value and for a key
        rows += [
            ("TREG_SET", R("TREG", "SET", "big", b"v" * BIG, 1)),
            ("HOST", R("TREG", "SET", "big", b"v" * (BIG + 1), 1)),
            ("HOST", R("TREG", "GET", b"k" * (BIG + 1))),
        ]
    return [b for _, b in rows], [k for k, _ in rows]


# ---- values that look like framing ----
FAKE = R("TREG", "SET", "evil", "x", 99)  # a well-formed command, carried as a value


def tricky():
    """binary-safe values: a whole fake command; '$' and '*' right where the
    next token would start if a length were one off; a value longer than two
    workgroups' bytes (256 lanes a workgroup, a byte a lane) full of '*1\\r\\n$1\\r\\nx\\r\\n'"""
    long_value = b"*1\r\n$1\r\nx\r\n" * 120  # 1,320 bytes
    return [
        R("TREG", "SET", "a", FAKE, 1) + R("TREG", "GET", "a"),
        R("TLOG", "INS", "b", b"\r\n$3\r\nabc\r\n*2\r\n", 2),
        R("TLOG", "INS", "c", b"$", 3) + R("TLOG", "INS", "c", b"*", 4),
        R("TREG", "SET", "d", b"*3\r\n$4\r\nTREG\r\n$3\r\nGET\r\n$1\r\nd", 5),  # ends where a fake command would
        R("TREG", "SET", "e", long_value, 6) + R("TREG", "GET", "e"),
        R("GCOUNT", "INC", FAKE, 7),  # a key that is a command
    ]


# ---- the doubling's round boundaries ----
TOKEN_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 1025)


def with_tokens(t):
    """one connection of exactly t tokens: a header and t - 1 words"""
    words = ["GCOUNT", "GET", "k"][:t - 1]
    words += ["w%d" % i for i in range(t - 1 - len(words))]
    return R(*words)


def round_boundaries():
    """connections of TOKEN_COUNTS tokens, an empty connection among them, and
    the same token counts made of several commands"""
    out = [with_tokens(t) for t in TOKEN_COUNTS]
    out.insert(3, b"")
    out.append(R("TREG", "GET", "k") * 16)          # 64 tokens in 16 commands
    out.append(R("TREG", "GET", "k") * 16 + R())    # 65
    out.append(R("TLOG", "SIZE", "k") * 256 + R())  # 1,025
    return out


# ---- token starts at every residue mod 8 ----
def residues():
    """keys of 0 .. 15 bytes move every later token along: one connection"""
    return [b"".join(R("TREG", "SET", "k" * n, "v" * (n % 5), n) for n in range(16))]


# ---- phases ----
def phases():
    alt = b"".join(R("TREG", "SET", "p", "v%d" % i, i) + R("TREG", "GET", "p") + R("TLOG", "INS", "p", "e%d" % i, i) +
                   R("TLOG", "GET", "p") for i in range(1, 6))
    a = R("GCOUNT", "INC", "x", 1) + R("GCOUNT", "INC", "y", 2) + R("GCOUNT", "GET", "x") + R("SYSTEM", "GETLOG") + \
        R("SYSTEM", "GETLOG") + R("GCOUNT", "GET", "y")
    b = R("GCOUNT", "GET", "x") + R("PNCOUNT", "DEC", "z", 3) + R("PNCOUNT", "INC", "z", 1) + R("PNCOUNT", "GET", "z")
    return [alt, a, b]


# ---- pipelining ----
def pipelined(ncmd=20000, nsingle=300, big=1 << 20):
    """one connection of ncmd pipelined commands beside nsingle single-command
    connections, and one command carrying a value of `big` bytes"""
    pipe = b"".join(R("TREG", "SET", "k%d" % (i % 997), "value-%d" % i, i) if i % 3 else R("TREG", "GET", "k%d" % (i % 997))
                    for i in range(ncmd))
    singles = [R("TLOG", "INS", "log%d" % (i % 50), "entry %d" % i, i) for i in range(nsingle)]
    fake = b"*2\r\n$3\r\nGET\r\n"
    value = (fake * (big // len(fake) + 1))[:big]
    return singles[:nsingle // 2] + [pipe] + singles[nsingle // 2:] + [R("TREG", "SET", "huge", value, 1) + R("TREG", "GET", "huge")]


# ---- the docs' sessions (tests/golden/kat_docs.json) as requests ----
def doc_requests(kat, name, typ):
    """-> [(request bytes, its words, expected reply as the docs print it)];
    the fixture writes `GET key 1` as the op "GET1\""""
    out = []
    for step in kat[name]["steps"]:
        *words, expect = step
        if words[0] == "GET1":
            words = ["GET", words[1], 1]
        words = [typ] + [str(w) for w in words]
        out.append((R(*words), words, expect))
    return out
