"""The UJSON render in stored order without a GPU: the host rule
(ujson_doc.render_stored_order) against render, the rules of
jylis_amd/csrc/jy_uj_render.hpp as plain C++ over the same leaf sets
(tests/uj_render_check.cpp, under the sanitizers), and the new entry point in
the header, the Python binding and the Pony FFI."""
import itertools
import os
import re
import shutil
import struct
import subprocess

import pytest

from jylis_amd import ujson_doc as U
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the adversarial alphabet: the stored length word is little-endian, so keys of
# 1, 2, 255 and 256 bytes do not sort by length; "1" is a proper prefix of "12"
KEYS = ["a", "b", "ab", "k" * 255, "q" * 256, "z"]
VALUES = ["1", "12", '"x"']
PATHS = ([()] + [(k,) for k in KEYS] + [(a, b) for a in KEYS[:3] for b in (KEYS[0], KEYS[2], KEYS[4])]
         + [("a", "b", "a"), ("a", "a", "b"), ("ab", "a", "z"), (KEYS[3], KEYS[4], KEYS[5])])
LEAVES = [(p, v) for p in PATHS for v in VALUES]

# hand-written renders: the primer's cases (ujson.md:134-170) and each node shape
HAND = [
    ([], ""),
    ([((), "1")], "1"),                                               # a bare value
    ([((), "2"), ((), "1"), ((), "12")], "[1,12,2]"),                 # a set, by the bytes of the text
    ([(("b",), "2"), (("a",), "1")], '{"a":1,"b":2}'),                # a map
    ([((), "2"), (("k",), "1")], '[{"k":1},2]'),                      # a map and values at one node
    ([(("a", "b", "c"), "1")], '{"a":{"b":{"c":1}}}'),                # nesting three deep
    ([(("a", "b", "c"), "1"), (("a", "b"), "2"), (("a",), "3"), ((), "4")], '[{"a":[{"b":[{"c":1},2]},3]},4]'),
    ([(("roles",), '"user"'), (("roles",), '"admin"')], '{"roles":["admin","user"]}'),
    ([(("roles",), '"user"')], '{"roles":"user"}'),                   # a set of one is no set
    ([((), "1"), ((), "1")], "1"),                                    # a rose is a rose
    ([(("a",), "1"), (("b",), "2"), ((), "3"), ((), "4")], '[{"a":1,"b":2},3,4]'),  # at most one map in a set
    # the length word's bytes sort first: 256 (00 01 00 00) < "z" (01 ..) < "ab" (02 ..) < 255 (FF 00 ..)
    ([(("ab",), "1"), (("z",), "2"), (("q" * 256,), "3"), (("k" * 255,), "4")],
     '{"%s":3,"z":2,"ab":1,"%s":4}' % ("q" * 256, "k" * 255)),
    ([(("a",), "12"), (("a",), "1"), (("a", "a"), "1")], '{"a":[{"a":1},1,12]}'),
    ([(("x", "y"), "1"), (("x", "z"), "2"), (("w",), "3")], '{"w":3,"x":{"y":1,"z":2}}'),
    ([(("ü",), '"é"'), ((" ",), "null"), (("\x7f",), "true")], '{" ":null,"\x7f":true,"ü":"é"}'),
]


def subsets():
    """every leaf set of up to 2 leaves of the alphabet, and a fixed stride of the 3- and 4-leaf ones"""
    for size in (0, 1, 2):
        yield from itertools.combinations(LEAVES, size)
    for size, stride in ((3, 11), (4, 997)):
        yield from itertools.islice(itertools.combinations(LEAVES, size), 0, None, stride)


def test_alphabet_is_adversarial():
    enc = sorted(U.encode_path((k,)) for k in KEYS)
    by_len = sorted((U.encode_path((k,)) for k in KEYS), key=lambda e: (len(e), e))
    assert enc != by_len  # the byte order of the length word is not the numeric order
    assert U._encode((), "12").startswith(U._encode((), "1"))  # a proper prefix
    assert {len(p) for p in PATHS} == {0, 1, 2, 3}
    assert {len(k) for k in KEYS} >= {1, 2, 255, 256}


def test_stored_order_renders_what_render_renders():
    n = 0
    for leaves in subsets():
        leaves = list(leaves)
        got = U.render_stored_order(leaves)
        assert U.canonical(got) == U.canonical(U.render(leaves)), (leaves, got)
        assert got == U.render_stored_order(leaves[::-1] + leaves[:1])  # order and repeats of the input do not matter
        n += 1
    assert n > 5000


@pytest.mark.parametrize("leaves,text", HAND, ids=[t[:24] or "empty" for _, t in HAND])
def test_hand_written(leaves, text):
    assert U.render_stored_order(leaves) == text
    assert U.canonical(text) == U.canonical(U.render(leaves))


def test_depth_and_key_rules_match_the_header():
    src = open(os.path.join(ROOT, "jylis_amd", "csrc", "jy_uj_render.hpp")).read()
    depth = int(re.search(r"kRenderDepth = (\d+);", src).group(1))
    hdr = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    assert depth in (31, 63) and int(re.search(r"JY_UJSON_RENDER_DEPTH = (\d+)", hdr).group(1)) == depth
    deep = [(tuple("k" for _ in range(depth + 2)), "1"), (tuple("k" for _ in range(depth)), "2")]
    assert U.canonical(U.render_stored_order(deep)) == U.canonical(U.render(deep))  # the host rule has no limit


def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(cc) if cc else None
        if path:
            return path
    return None


def case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for leaves, text in cases:
            f.write(struct.pack("<I", len(leaves)))
            for p, v in leaves:
                e = U._encode(tuple(p), v)
                f.write(struct.pack("<I", len(e)) + e)
            t = text.encode()
            f.write(struct.pack("<I", len(t)) + t)


def test_rules_stand_alone(tmp_path):
    """leaf_cmp, leaf_shape, common_segments, mask_compose and leaf_text run
    sequentially over the subsets and the hand-written cases, under the address
    and undefined-behaviour sanitizers, byte for byte against render_stored_order"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "uj_render_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "uj_render_check.cpp")],
                   check=True)
    cases = [(list(l), U.render_stored_order(list(l))) for l in subsets()]
    cases += [(l + l[:1], t) for l, t in HAND]  # (with a duplicate leaf)
    deep = [(tuple("k%d" % (i % 3) for i in range(d)), v) for d in (29, 30, 31) for v in VALUES]
    cases.append((deep, U.render_stored_order(deep)))
    cases_path = str(tmp_path / "cases.bin")
    case_file(cases_path, cases)
    out = subprocess.run([exe, cases_path], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok %d" % len(cases), out.stdout[-2000:] + out.stderr[-4000:]


def test_new_symbol_is_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    name, arity = "jy_ujson_get_resp", 13
    assert hdr.get(name) == arity, hdr.get(name)
    assert len(_lib.SIGNATURES[name][1]) == arity
    assert pony.get(name) == arity, pony.get(name)
