"""UJSON path reads without a GPU: the property jy_ujson_path_read's byte
compare rests on -- encode_path(p) is a byte prefix of a leaf's encoding iff p
is a prefix of the leaf's path -- checked exhaustively over an adversarial
segment alphabet; _encode's bytes unchanged by its rewrite; the call declared
alike in the header, the ctypes table and the Pony FFI."""
import itertools
import os

from jylis_amd import ujson_doc as U
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# segments: the empty one, string prefixes of each other, one whose bytes read
# as a length word plus a byte (01 00 00 00 61), and the word loop's tails
SEGMENTS = ["", "a", "ab", "abc", "\x01\x00\x00\x00a", "s" * 7, "s" * 8, "s" * 9]
# values: empty, and texts that begin like a length word (of 1, of 0) or like a segment
VALUES = ["", "\x01\x00\x00\x00a", "\x00\x00\x00\x00", "a"]


def _paths(depth):
    return [p for d in range(depth + 1) for p in itertools.product(SEGMENTS, repeat=d)]


def test_the_segment_alphabet_is_what_it_claims():
    assert SEGMENTS[4].encode() == bytes([1, 0, 0, 0, 0x61])
    assert [len(s.encode()) for s in SEGMENTS[5:]] == [7, 8, 9]
    assert VALUES[1].encode()[:4] == (1).to_bytes(4, "little")


def test_encoded_path_is_a_byte_prefix_iff_it_is_a_path_prefix():
    paths = _paths(3)
    encoded = [(p, U.encode_path(p)) for p in paths]
    assert len(paths) == 1 + 8 + 64 + 512
    hits = 0
    for q in paths:
        for v in VALUES:
            leaf = U._encode(q, v)
            for p, ep in encoded:
                is_prefix = q[:len(p)] == p
                assert leaf.startswith(ep) == is_prefix, (p, q, v)
                # what the kernel also asks: the terminator lies behind the path
                assert not is_prefix or len(ep) + 4 <= len(leaf)
                hits += is_prefix
    assert hits == sum(len(q) + 1 for q in paths) * len(VALUES)


def test_encode_is_unchanged():
    # the leaves of test_ujson_doc.py::test_leaf_handles_stable, by the formula written out
    def old_encode(path, value):
        b = bytearray()
        for p in path:
            e = p.encode()
            b += len(e).to_bytes(4, "little") + e
        b += b"\xff\xff\xff\xff" + value.encode()
        return bytes(b)
    t = U.LeafTable()
    for path, value in [(("x", "y"), '"v"'), (("xy",), '"v"'), ((), "0"), (("ключ", "é"), '"日本語"')]:
        assert U._encode(path, value) == old_encode(path, value)
        assert U._encode(path, value) == U.encode_path(path) + b"\xff\xff\xff\xff" + value.encode()
        assert t.handle(path, value) == (U._fnv1a64(old_encode(path, value)) or 1)
        assert U._decode(U._encode(path, value)) == (path, value)
    assert U._encode(("x", "y"), '"v"') == bytes.fromhex("0100000078" "0100000079" "ffffffff" "227622")
    assert U.encode_path(()) == b"" and U.encode_path(("ab",)) == bytes.fromhex("020000006162")


def test_the_call_is_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    name = "jy_ujson_path_read"
    assert name in hdr and name in pony and name in _lib.SIGNATURES
    assert hdr[name] == pony[name] == len(_lib.SIGNATURES[name][1]) == 14
    assert _lib.SIGNATURES[name][0] is _lib.I32
    text = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    assert "#define JY_PATH_LEAVES 1u" in text and _lib.PATH_LEAVES == 1
    flat = " ".join(text.split()).replace(" * ", " ")
    assert "jy_node_lock_type(node, JY_UJSON), NEVER under JY_NODE_NOFENCE, as the leaf store calls above" in flat
    assert "host compositions of RM / INS" not in flat
