"""UJSON GET as a keyed kind of the RESP decoder, without a GPU: the reference
(tests/resp_ujson_cases.py) against literals, the rule as plain C++
(jylis_amd/csrc/jy_resp_in.hpp through tests/resp_ujson_check.cpp, built with
the address and undefined-behaviour sanitizers and run as a program of its own)
against the reference, the declarations of the new calls, and what the case
generators cover, so that a GPU pass means something."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resp_in_cases as RC
import resp_in_ref as ref
import resp_ujson_cases as UC
from resp_in_ref import request as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(buf, flags=UC.FLAG):
    return UC.decode(buf, np.array([0, len(buf)], np.uint64), flags)


# ---- 1. the reference ----
def test_path_encoding_is_the_path_reads():
    from jylis_amd.ujson_doc import encode_path
    for path in ((), ("a",), ("", "b"), ("contact", "email"), ("x" * 300, "y")):
        assert UC.encode_path([p.encode() for p in path]) == encode_path(path)
    assert UC.encode_path([b"ab", b""]) == b"\x02\0\0\0ab\0\0\0\0"
    assert encode_path((b"\xff\r\n",)) == b"\x03\0\0\0\xff\r\n"  # segments may be bytes


def test_reference_literals():
    buf = R("UJSON", "GET", "doc", "contact", "email")
    d = _one(buf)
    assert d["sizes"] == [1, 5, 1, 3, 4 + 7 + 4 + 5, 1]
    assert d["cmd_kind"].tolist() == [UC.UJSON_GET] and d["num"].tolist() == [0] and d["op"].tolist() == [0]
    assert bytes(d["key_bytes"]) == b"doc"
    assert bytes(d["val_bytes"]) == b"\x07\0\0\0contact\x05\0\0\0email"
    assert d["group_class"].tolist() == [UC.UJSON_GET]
    # the whole document: an empty value
    d = _one(R("UJSON", "GET", "doc"))
    assert d["sizes"] == [1, 3, 1, 3, 0, 1] and d["val_offs"].tolist() == [0, 0]
    # without the flag it is resp_in_ref's decode, array by array
    for bufs in (UC.with_ujson_commands(), RC.phases() + RC.tricky()):
        b, offs = ref.join(bufs)
        want, got = ref.decode(b, offs), UC.decode(b, offs, 0)
        assert want.keys() == got.keys()
        for name in want:
            np.testing.assert_array_equal(np.asarray(want[name]), np.asarray(got[name]), err_msg=name)


def test_phase_table():
    """UJSON SET | UJSON GET | UJSON GET | TREG GET | UJSON GET, and the same commands in another order"""
    b, offs = ref.join(UC.phases())
    d = UC.decode(b, offs, UC.FLAG)
    H, G, T = ref.HOST, UC.UJSON_GET, ref.TREG_GET
    assert d["cmd_kind"].tolist() == [H, G, G, T, G, T, G, H, G, G]
    assert d["cmd_phase"].tolist() == [0, 1, 1, 2, 3, 0, 1, 2, 3, 3]
    assert d["group_phase"].tolist() == [0, 1, 2, 3] and d["group_class"].tolist() == [T, G, T, G]
    assert d["row_cmd"].tolist() == [5, 1, 2, 6, 3, 4, 8, 9]
    # without the flag the GETs are HOST commands like the SET: fewer phases
    assert UC.decode(b, offs, 0)["cmd_phase"].tolist() == [0, 0, 0, 1, 2, 0, 1, 1, 1, 1]


# ---- 2. the rule as plain C++ ----
def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cc) if cc else None
        if path:
            return path
    return None


def test_rule_stand_alone(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "resp_ujson_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "resp_ujson_check.cpp")],
                   check=True)
    cases = UC.rule_cases()
    lines = []
    for _, head, lens, flags in cases:
        hexes = [h.hex() or "-" for h in head]
        lines.append(" ".join(map(str, [flags, len(lens), *lens, len(hexes), *hexes])))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for (name, head, lens, flags), g in zip(cases, got):
        kind, op, num, ki, vi = UC.classify_lens(head, lens, flags)
        want = (kind, op, num, -1 if ki is None else ki, -1 if vi is None else vi, 1)
        assert g == want, (name, g, want)


# ---- 3. what the cases cover ----
def test_rule_cases_cover():
    cases = {name: UC.classify_lens(head, lens, flags)[0] for name, head, lens, flags in UC.rule_cases()}
    nk = len(RC.kinds(with_big=False)[0])
    for i in range(nk):  # the flag changes no existing case but the one UJSON GET among them
        a, b = cases["kinds%d/0" % i], cases["kinds%d/1" % i]
        assert a == b or (a, b) == (ref.HOST, UC.UJSON_GET), i
    assert sum(cases["kinds%d/0" % i] != cases["kinds%d/1" % i] for i in range(nk)) == 1
    assert {cases["kinds%d/0" % i] for i in range(nk)} == set(range(10))
    G, H = UC.UJSON_GET, ref.HOST
    assert cases["get-off"] == H and cases["get-2-words"] == H
    assert cases["get-whole"] == G and cases["get-path"] == G
    assert cases["get-lower-op"] == H and cases["get-lower-type"] == H
    assert all(cases["write-" + op] == H for op in ("SET", "CLR", "INS", "RM"))
    assert (cases["key-max"], cases["key-over"]) == (G, H)
    assert (cases["seg3-max"], cases["seg3-over"], cases["seg7-max"], cases["seg7-over"]) == (G, H, G, H)
    by = {name: lens for name, _, lens, _ in UC.rule_cases()}
    assert by["seg7-over"][7] == UC.MAX + 1 and 7 >= UC.WORDS_READ and max(by["seg7-over"][:7]) <= UC.MAX
    assert by["seg3-over"][3] == UC.MAX + 1 and by["key-over"][2] == UC.MAX + 1


def test_decoder_inputs_cover():
    consts = open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_resp_in.hpp")).read()
    assert int(re.search(r"kWordsRead = (\d+);", consts).group(1)) == UC.WORDS_READ
    assert int(re.search(r"kPathWord0 = (\d+);", consts).group(1)) == 3
    kthreads = int(re.search(r"constexpr int kThreads = (\d+);",
                             open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_wire.hpp")).read()).group(1))
    # path lengths at the edges of the words a command lane reads (2 segments end at word 5) and of a wave
    d = UC.decode(*ref.join(UC.path_word_counts()), UC.FLAG)
    assert np.diff(d["cmd_word_offs"].astype(np.int64)).tolist() == [3 + n for n in UC.PATH_WORDS]
    assert {0, 1, 2, 5, 6, 63, 64, 65} == set(UC.PATH_WORDS) and (d["cmd_kind"] == UC.UJSON_GET).all()
    # segment lengths around the gather's 8-byte loads
    d = UC.decode(*ref.join(UC.segment_lengths()), UC.FLAG)
    assert sorted(set(d["word_len"][d["word_len"] != 5].tolist()) - {3, 1}) == [0, 7, 8, 9, 255]
    # framing bytes inside segments
    d = UC.decode(*ref.join(UC.binary_segments()), UC.FLAG)
    assert not d["conn_err"].any() and (d["cmd_kind"] == UC.UJSON_GET).all()
    vals = bytes(d["val_bytes"])
    for s in (b"\r\n", b"\0", b"\xff", b"$3\r\n", b"*1\r\n"):
        assert s in UC.BINARY and len(s).to_bytes(4, "little") + s in vals
    # path words on both sides of a workgroup's edge, in tokens and in commands
    bufs = UC.block_edge(kthreads)
    d = UC.decode(*ref.join(bufs), UC.FLAG)
    assert d["sizes"][0] > kthreads // 2 and d["sizes"][1] > 2 * kthreads
    assert {UC.UJSON_GET, ref.TREG_SET} == set(d["cmd_kind"].tolist())
    # the cuts: used stops before the cut command, only the malformed token closes
    for buf, used, closed in UC.cuts():
        d = _one(buf)
        assert (int(d["conn_used"][0]), bool(d["conn_err"][0]), d["sizes"][0]) == (used, closed, 1)


# ---- 4. the declarations ----
def test_declarations():
    from jylis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    pony = open(os.path.join(ROOT, "pony", "jylis_gpu", "ffi.pony")).read()
    assert re.search(r"JY_CMD_UJSON_GET = 10,", hdr) and re.search(r"JY_CMD_NKINDS = 11\b", hdr)
    assert "ONLY under JY_RESP_UJSON_GET" in hdr and "jy_node_lock_type(node, JY_UJSON)" in hdr
    assert _lib.CMD_UJSON_GET == UC.UJSON_GET and _lib.RESP_UJSON_GET == UC.FLAG
    for name, arity in (("jy_resp_decode_opts", 27), ("jy_resp_exec_opts", 10)):
        m = re.search(r"int32_t %s\(([^;]*)\);" % name, hdr)
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["jy_resp_decode_opts"][1]) == len(_lib.SIGNATURES["jy_resp_decode"][1]) + 1
    assert "use @jy_resp_exec_opts[I32](" in pony


# ---- 5. the Python layer ----
def test_leaves_lock_is_taken_once_per_thread():
    """UJSONDocs.resp_exec holds the leaf store's lock while its callback's calls
    enter it again: the constructor's lock is taken once, and is free afterwards"""
    import threading
    from jylis_amd import ujson_doc as U
    real, taken = threading.Lock(), []

    class _Lock:
        def __enter__(self):
            assert real.acquire(timeout=5)
            taken.append(threading.get_ident())

        def __exit__(self, *a):
            real.release()
    dl = U.DeviceLeaves(object(), lock=_Lock)
    with dl.lock():
        with dl.lock():
            with dl.lock():
                assert real.locked()
        assert real.locked() and len(taken) == 1
        seen = []
        t = threading.Thread(target=lambda: seen.append(real.acquire(blocking=False)))  # another thread finds it held
        t.start()
        t.join()
        assert seen == [False]
    assert not real.locked() and len(taken) == 1
    with dl.lock():
        assert len(taken) == 2


def test_apply_words():
    from jylis_amd import ujson_doc as U
    calls = []

    class _Docs(U.UJSONDocs):
        def get_resp(self, keys, paths):
            calls.append(("GET", keys, paths))
            return [b"$0\r\n\r\n"]

        def set(self, key, path, text):
            calls.append(("SET", key, path, text))

        def clr(self, key, path=()):
            calls.append(("CLR", key, path))
    d = _Docs(None, 1)
    assert d.apply([b"UJSON", b"GET", b"k", b"a", b"b"]) == b"$0\r\n\r\n"
    assert d.apply([b"UJSON", b"SET", b"k", b"a", b"1"]) == b"+OK\r\n" == d.apply([b"UJSON", b"CLR", b"k"])
    assert d.apply([b"UJSON", b"GET", b"\xffk", b"\xfe"]) == b"$0\r\n\r\n"  # binary-safe: passed on as bytes
    assert calls == [("GET", ["k"], [("a", "b")]), ("SET", "k", ("a",), "1"), ("CLR", "k", ()),
                     ("GET", [b"\xffk"], [(b"\xfe",)])]
    for bad in ([b"UJSON", b"NOPE", b"k"], [b"UJSON", b"SET", b"k"], [b"UJSON", b"GET"], [b"TREG", b"GET", b"k"],
                [b"UJSON", b"SET", b"\xffk", b"1"]):
        with pytest.raises(ValueError):
            d.apply(bad)
