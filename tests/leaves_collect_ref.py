"""A numpy restatement of jy_ujson_leaves_collect, the yardstick of
tests/test_ujson_leaves_collect_cpu.py and _gpu.py (the reference has no leaf
store: Pony's GC plays that part).

The live set is the union of the `elems` of the state (state_wire over every
slot), the `elems` of the pending deltas (what the next flush_wire returns)
and the caller's `keep`; a stored leaf whose handle is live is kept, and it
owns its length rounded up to 8 in the arena."""
import numpy as np


def rounded(n):
    return (int(n) + 7) // 8 * 8


def live_set(state_elems, pending_elems=(), keep=()):
    """the handles collect keeps alive (handle 0 in `keep` is ignored)"""
    live = set(int(h) for h in np.asarray(state_elems, np.uint64))
    live |= set(int(h) for h in np.asarray(pending_elems, np.uint64))
    live |= set(int(h) for h in np.asarray(list(keep), np.uint64) if int(h) != 0)
    return live


def collect(stored, state_elems, pending_elems=(), keep=()):
    """stored {handle: encoding}, what the store holds -> (out6, kept {handle:
    encoding}).  out6 = (leaves kept, arena bytes kept, leaves dropped, arena
    bytes dropped, live elements examined whose handle has no stored leaf,
    keep handles with no stored leaf); the last two count every element and
    every keep entry, repeats repeated, handle 0 of `keep` never."""
    live = live_set(state_elems, pending_elems, keep)
    kept = {h: e for h, e in stored.items() if h in live}
    nbytes = lambda t: sum(rounded(len(e)) for e in t.values())
    examined = [int(h) for part in (state_elems, pending_elems) for h in np.asarray(part, np.uint64)]
    no_leaf = sum(1 for h in examined if h not in stored)
    keep_no_leaf = sum(1 for h in np.asarray(list(keep), np.uint64) if int(h) != 0 and int(h) not in stored)
    return (len(kept), nbytes(kept), len(stored) - len(kept), nbytes(stored) - nbytes(kept), no_leaf,
            keep_no_leaf), kept
