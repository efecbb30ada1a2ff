"""UJSON INS / RM / CLR by key string, without a GPU: the value rule against
ujson_doc.canonical_value, the rule and the classification as plain C++
(jylis_amd/csrc/jy_resp_in.hpp through tests/ujson_put_check.cpp, built with the
address and undefined-behaviour sanitizers and run as a program of its own)
against the reference of tests/ujson_put_cases.py, the declarations of the new
calls, and what the case generators cover, so that a GPU pass means something."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resp_in_ref as ref
import resp_ujson_cases as UC
import ujson_put_cases as PC
from resp_in_ref import request as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the value rule ----
def test_value_rule_literals():
    for w in PC.ACCEPTED:
        assert PC.value_plain(w), w
    for w in PC.REJECTED:
        assert not PC.value_plain(w), w
    assert len(PC.PRINTABLE) == 2 + 95 - 2 and len(PC.ACCEPTED[5]) == 255 and len(PC.REJECTED[12]) == 256
    assert PC.REJECTED[:13] == [b"-0", b"01", b"1.0", b"1e3", b" 1", b"1 ", b"9" * 19, b'"a\\"b"', b'"', b"tru", b"",
                                b'"a\x7fb"', b'"' + b"x" * 254 + b'"']


def test_value_rule_against_canonical_value():
    """every word the rule accepts is its own canonical text, so copying it is canonicalising it"""
    from jylis_amd.ujson_doc import canonical_value
    words = PC.ACCEPTED + PC.REJECTED + PC.random_words(1, 60000, 10) + PC.random_words(2, 20000, 24)
    accepted = [w for w in words if PC.value_plain(w)]
    kinds = {w[:1] for w in accepted}
    assert len(accepted) > 2000 and {b'"', b"-"} <= kinds and any(k.isdigit() for k in kinds)
    for w in accepted:
        assert canonical_value(w.decode()) == w.decode(), w
    # the rule is conservative, not exact: some rejected words are valid JSON the host canonicalises
    assert canonical_value("1.0") == "1.0" and canonical_value("-0") == "0" and canonical_value("1e3") == "1000.0"


def test_leaf_encoding_is_the_leaf_stores():
    from jylis_amd.ujson_doc import _encode
    for path, v in (((), "1"), (("a",), '"x"'), (("", "b"), "null"), (("contact", "email"), '"a@b"')):
        assert PC.encode_leaf([p.encode() for p in path], v.encode()) == _encode(path, v)
    assert PC.encode_leaf([b"ab"], b"7") == b"\x02\0\0\0ab\xff\xff\xff\xff7"


# ---- 2. the reference ----
def _one(buf, flags=PC.FLAG_WRITE):
    return PC.decode(buf, np.array([0, len(buf)], np.uint64), flags)


def test_reference_literals():
    d = _one(PC.ins("doc", "contact", "email", '"a@b"'))
    assert d["sizes"] == [1, 6, 1, 3, 11 + 9 + 4 + 5, 1]
    assert d["cmd_kind"].tolist() == [PC.UJSON_WRITE] and d["op"].tolist() == [PC.INS] and d["num"].tolist() == [0]
    assert bytes(d["val_bytes"]) == b'\x07\0\0\0contact\x05\0\0\0email\xff\xff\xff\xff"a@b"'
    d = _one(PC.rm("doc", "7") + PC.clr("doc"))
    assert d["op"].tolist() == [PC.RM, PC.CLR] and d["val_offs"].tolist() == [0, 5, 5]
    assert bytes(d["val_bytes"]) == b"\xff\xff\xff\xff7"
    # without the write flag the reference is the parent's, array by array
    b, offs = ref.join(PC.all_inputs())
    for flags in (0, PC.FLAG_GET):
        want, got = UC.decode(b, offs, flags), PC.decode(b, offs, flags)
        assert want.keys() == got.keys()
        for name in want:
            np.testing.assert_array_equal(np.asarray(want[name]), np.asarray(got[name]), err_msg=name)
    assert (PC.decode(b, offs, 2)["cmd_kind"] == PC.UJSON_WRITE).sum() > 300


def test_phase_table():
    """UJSON INS | SET | GET | RM | CLR | CLR path | INS 1.0 on one connection"""
    b, offs = ref.join(PC.phases())
    H, W, G = ref.HOST, PC.UJSON_WRITE, UC.UJSON_GET
    d = PC.decode(b, offs, 3)
    assert d["cmd_kind"].tolist() == [W, H, G, W, W, H, H, H, H, W, W, G, H, W]
    assert d["cmd_phase"].tolist() == [0, 1, 2, 3, 3, 4, 4, 0, 0, 1, 1, 2, 3, 4]
    d = PC.decode(b, offs, 2)  # the GET is the host's: INS | SET GET | RM CLR | ...
    assert d["cmd_kind"].tolist()[:7] == [W, H, H, W, W, H, H] and d["cmd_phase"].tolist()[:7] == [0, 1, 1, 2, 2, 3, 3]


# ---- 3. the rule as plain C++ ----
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
    exe = str(tmp_path / "ujson_put_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "ujson_put_check.cpp")],
                   check=True)
    cases = PC.rule_cases()
    lines = []
    for _, words, lens, flags in cases:
        hexes = ["?" if w is None else (bytes(w).hex() or "-") for w in words]
        lines.append(" ".join(map(str, [flags, len(lens), *lens, *hexes])))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    flat = lambda c: (c[0], c[1], c[2], -1 if c[3] is None else c[3], -1 if c[4] is None else c[4])
    for (name, words, lens, flags), g in zip(cases, got):
        head = [w if w is not None else b"" for w in words[:PC.WORDS_READ]]
        want = flat(PC.case_classify(words, lens, flags))
        assert g[:5] == want, (name, g, want)
        # flags 0 and the GET flag alone: what the rule gave before the write kind existed
        assert g[5:10] == flat(UC.classify_lens(head, lens, 0)), name
        assert g[10:15] == flat(UC.classify_lens(head, lens, 1)), name
        assert g[15] == 1
        if words and words[-1] is not None:
            assert g[16] == int(PC.value_plain(words[-1])), (name, words[-1])


# ---- 4. what the cases cover ----
def test_rule_cases_cover():
    cases = {name: (PC.case_classify(words, lens, flags), words, lens) for name, words, lens, flags in PC.rule_cases()}
    kind = lambda name: cases[name][0][0]
    W, H = PC.UJSON_WRITE, ref.HOST
    nv = len(PC.ACCEPTED + PC.REJECTED) + 40
    for at in PC.VALUE_AT:  # the value at words 3, 4, 5 and 9: every accepted literal is a write, no rejected one
        for vi in range(nv):
            for op, code in (("INS", PC.INS), ("RM", PC.RM)):
                c, words, _ = cases["%s-at%d-v%d" % (op, at, vi)]
                assert len(words) == at + 1
                assert c[:2] == ((W, code) if PC.value_plain(words[-1]) else (H, 0)), (op, at, vi)
    assert min(PC.VALUE_AT) == 3 and 4 < PC.WORDS_READ <= 5 and max(PC.VALUE_AT) > PC.WORDS_READ
    assert sum(kind("INS-at9-v%d" % vi) == W for vi in range(nv)) >= len(PC.ACCEPTED)
    for flags in (0, 1):
        assert all(kind("off-%s/%d" % (op, flags)) == H for op in ("INS", "RM", "CLR", "SET"))
    assert kind("off-GET/0") == H and kind("off-GET/1") == UC.UJSON_GET
    assert cases["clr"][0][:2] == (W, PC.CLR)
    assert [kind(n) for n in ("clr-path", "clr-2-words", "set", "ins-3-words", "ins-lower", "get-write-only")] == [H] * 6
    assert kind("get-both") == UC.UJSON_GET
    assert [kind(n) for n in ("key-max", "key-over", "seg3-over", "seg7-over")] == [W, H, H, H]
    assert [kind(n) for n in ("leaf-max", "leaf-over", "leaf7-max", "leaf7-over")] == [W, H, W, H]
    assert sum(4 + x for x in cases["leaf7-max"][2][3:]) == PC.MAX == (1 << 24) - 1


def test_decoder_inputs_cover():
    consts = open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_resp_in.hpp")).read()
    assert int(re.search(r"kWordsRead = (\d+);", consts).group(1)) == PC.WORDS_READ
    assert int(re.search(r"kUjValueMax = (\d+);", consts).group(1)) == PC.VALUE_MAX
    kthreads = int(re.search(r"constexpr int kThreads = (\d+);",
                             open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_wire.hpp")).read()).group(1))
    W = PC.UJSON_WRITE
    d = PC.decode(*ref.join(PC.path_word_counts()), 2)
    assert (d["cmd_kind"] == W).all()
    assert np.diff(d["cmd_word_offs"].astype(np.int64)).tolist() == sum(([4 + n, 4 + n, 3] for n in PC.PATH_WORDS), [])
    assert set(PC.PATH_WORDS) == {0, 1, 4, 65}
    d = PC.decode(*ref.join(PC.value_lengths()), 2)
    rows = np.diff(d["val_offs"].astype(np.int64))
    assert {int(x) % 8 for x in rows} == set(range(8))       # leaf lengths on both sides of every multiple of 8
    vals = d["word_len"][d["cmd_word_offs"][1:].astype(np.int64) - 1]
    assert set(range(1, 18)) <= set(vals.tolist()) and {255, 256} <= set(vals.tolist())
    assert d["cmd_kind"].tolist()[-2:] == [W, ref.HOST]      # 255 bytes on the device, 256 the host's
    d = PC.decode(*ref.join(PC.binary_values()), 2)
    assert not d["conn_err"].any() and (d["cmd_kind"] == ref.HOST).sum() == 1
    for s in (b"$3\r\n", b"*1\r\n", b"\xff\xff\xff\xff"):
        assert len(s).to_bytes(4, "little") + s in bytes(d["val_bytes"])
    d = PC.decode(*ref.join(PC.block_edge(kthreads)), 2)
    assert d["sizes"][2] > kthreads + 30 and {W, ref.TREG_SET, ref.HOST} == set(d["cmd_kind"].tolist())
    assert {PC.INS, PC.RM, PC.CLR} <= set(d["op"].tolist())
    for buf, used, closed in PC.cuts():
        d = _one(buf)
        assert (int(d["conn_used"][0]), bool(d["conn_err"][0]), d["sizes"][0]) == (used, closed, 1)


# ---- 5. the declarations ----
def test_declarations():
    from jylis_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    pony = open(os.path.join(ROOT, "pony", "jylis_gpu", "ffi.pony")).read()
    assert re.search(r"JY_CMD_NKINDS = 11\b", hdr) and re.search(r"JY_CMD_UJSON_WRITE = 11,", hdr)
    assert re.search(r"JY_CMD_NKINDS_ALL = 12\b", hdr) and re.search(r"JY_RESP_UJSON_WRITE = 2\b", hdr)
    assert "ONLY under JY_RESP_UJSON_WRITE" in hdr and "UJSONDocs.apply" in hdr
    assert (_lib.CMD_UJSON_WRITE, _lib.CMD_NKINDS, _lib.CMD_NKINDS_ALL) == (PC.UJSON_WRITE, 11, 12)
    assert (_lib.RESP_UJSON_GET, _lib.RESP_UJSON_WRITE, _lib.UJ_VALUE_MAX) == (1, 2, PC.VALUE_MAX)
    assert (_lib.UJSON_INS, _lib.UJSON_RM, _lib.UJSON_CLR) == (PC.INS, PC.RM, PC.CLR)
    for name, arity in (("jy_ujson_write_keys", 9), ("jy_ujson_write_keys_info", 2)):
        m = re.search(r"int32_t %s\(([^;]*)\);" % name, hdr)
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert "use @%s[I32](" % name in pony
    import inspect
    from jylis_amd import engine, repo, resp_in, ujson_doc
    for fn in (engine.Engine.resp_decode, engine.Engine.resp_exec_raw, engine.Engine.resp_exec, resp_in.exec_resp,
               ujson_doc.UJSONDocs.resp_exec):
        assert inspect.signature(fn).parameters["ujson_write"].default is False, fn
    assert hasattr(engine.Engine, "ujson_write_keys_info") and hasattr(repo.RepoUJSON, "write_keys")
