"""A numpy restatement of "a UJSON wire batch with leaves" and small helpers
for the leaf store's tests (tests/test_ujson_leaves_cpu.py, _gpu.py)."""
import numpy as np

from jylis_amd import ujson_doc as U


def handle_of(encoding):
    """the handle formula: FNV-1a 64 over the encoding, 0 replaced by 1"""
    return U._fnv1a64(bytes(encoding)) or 1


def pack(items):
    """[bytes] -> (uint8 bytes, uint64 offs[n + 1]), packed back to back"""
    offs = np.zeros(len(items) + 1, np.uint64)
    if items:
        offs[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64)
    raw = b"".join(items)
    return np.frombuffer(raw, np.uint8).copy() if raw else np.zeros(0, np.uint8), offs


def unpack(item_bytes, item_offs):
    raw = np.asarray(item_bytes, np.uint8).tobytes()
    o = np.asarray(item_offs, np.uint64).astype(np.int64)
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def batch_leaves(elems, table):
    """leaf_bytes / leaf_offs[nel + 1] of a batch: item i = table[elems[i]], the
    encoded leaf of element i, one item per element (repeats repeated), an
    element the table does not hold an empty item"""
    return pack([table.get(int(h), b"") for h in np.asarray(elems, np.uint64)])


def leaf_of_length(n, path=()):
    """a (path, value) whose encoding has exactly n >= 4 bytes"""
    room = n - 4 - sum(4 + len(p.encode()) for p in path)
    assert room >= 0, (n, path)
    return tuple(path), "v" * room
