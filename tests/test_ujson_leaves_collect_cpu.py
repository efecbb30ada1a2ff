"""Collecting the UJSON leaf store, without a GPU: jy_ujson_leaves_collect is
declared alike in the header, the ctypes table and the Pony FFI; the header
states the keep rule, the lost-handle rule and the lock rule; the numpy
restatement (tests/leaves_collect_ref.py) on a hand-made state; the threshold
arithmetic of DeviceLeaves.maybe_collect against a stub engine."""
import os

import numpy as np

import leaves_collect_ref as CR
import leaves_ref as R
from jylis_amd import ujson_doc as U
from test_pony_glue import header_arity, pony_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "jy_ujson_leaves_collect"


def test_the_call_is_declared_alike():
    from jylis_amd import _lib
    hdr, pony = header_arity(), pony_decls()
    assert CALL in hdr and CALL in pony and CALL in _lib.SIGNATURES
    assert hdr[CALL] == pony[CALL] == len(_lib.SIGNATURES[CALL][1]) == 6
    assert _lib.SIGNATURES[CALL][0] is _lib.I32
    ffi = open(os.path.join(ROOT, "pony", "jylis_gpu", "ffi.pony")).read()
    assert "use @jy_ujson_leaves_collect[I32](" in ffi
    head = open(os.path.join(ROOT, "include", "jylis_gpu.h")).read()
    assert "#define JY_LEAVES_SHRINK 1u" in head and _lib.LEAVES_SHRINK == 1


def test_the_header_states_the_three_rules():
    text = " ".join(open(os.path.join(ROOT, "include", "jylis_gpu.h")).read().split()).replace(" * ", " ")
    # the keep rule
    assert "a caller that has put leaves and not yet written their elements passes their handles here" in text
    assert "Handle 0 in `keep` is ignored" in text
    # the lost-handle rule
    assert "a handle that was put but neither written into a document nor passed in `keep` loses its leaf; " \
           "putting the same leaf again restores it under the same handle" in text
    # the lock rule, and the older sentence that still holds for every leaf call
    assert "under a node the call is made under jy_node_lock_type(node, JY_UJSON), which waits for the queued " \
           "UJSON jobs whose leaves were already put" in text
    assert "jy_node_lock_type(node, JY_UJSON), NEVER under JY_NODE_NOFENCE" in text
    assert "The call is synchronising" in text and "the pending-delta store" in text


def test_the_restatement_on_a_hand_made_state():
    encs = [U._encode(*R.leaf_of_length(n)) for n in (4, 5, 8, 9, 17, 1000)]
    hs = [R.handle_of(e) for e in encs]
    stored = dict(zip(hs, encs))
    assert CR.rounded(4) == 8 and CR.rounded(8) == 8 and CR.rounded(9) == 16 and CR.rounded(0) == 0
    # the state holds leaf 0 twice and an opaque element; the pending delta leaf 2 and another
    # opaque one; keep names leaf 4, handle 0 and an unknown handle twice
    state = np.array([hs[0], 0xABCDEF, hs[0]], np.uint64)
    pending = np.array([hs[2], 0x1234], np.uint64)
    keep = [hs[4], 0, 0x777, 0x777]
    assert CR.live_set(state, pending, keep) == {hs[0], 0xABCDEF, hs[2], 0x1234, hs[4], 0x777}
    out6, kept = CR.collect(stored, state, pending, keep)
    assert kept == {hs[0]: encs[0], hs[2]: encs[2], hs[4]: encs[4]}
    assert out6 == (3, 8 + 8 + 24, 3, 8 + 16 + 1000, 2, 2)
    # nothing live: everything goes; everything live: nothing does
    assert CR.collect(stored, np.zeros(0, np.uint64)) == ((0, 0, 6, sum(CR.rounded(len(e)) for e in encs), 0, 0), {})
    out6, kept = CR.collect(stored, np.array(hs, np.uint64))
    assert kept == stored and out6[2:] == (0, 0, 0, 0)
    # an empty store under documents of opaque handles
    assert CR.collect({}, state)[0] == (0, 0, 0, 0, 3, 0)


class _StubEngine:
    """usage and collect as Engine has them: collect keeps `live` bytes of what is used"""

    def __init__(self):
        self.used, self.live, self.calls = 0, 0, []

    def ujson_leaves_usage(self):
        return (0, self.used, 1 << 30, 0)

    def ujson_leaves_collect(self, keep=None, shrink=False):
        from jylis_amd.engine import LeavesCollected
        self.calls.append((keep, shrink))
        dropped, self.used = self.used - self.live, self.live
        return LeavesCollected(1, self.live, 1, dropped, 0, 0)


def test_maybe_collect_threshold():
    eng = _StubEngine()
    dl = U.DeviceLeaves(eng)
    assert dl.auto_collect is False and dl.floor == 1 << 20 and dl.collections == 0
    floor = 1 << 20
    eng.used = floor  # nothing kept so far: used == 2 * 0 + floor is not above the threshold
    assert dl.maybe_collect() is None and eng.calls == []
    eng.used, eng.live = floor + 8, 4096
    got = dl.maybe_collect()
    assert got.kept_bytes == 4096 and got.dropped_bytes == floor + 8 - 4096
    assert eng.calls == [(None, False)] and dl.collections == 1
    eng.used = 2 * 4096 + floor  # equality with 2 x kept + floor: no collection
    assert dl.maybe_collect() is None and dl.collections == 1
    eng.used += 8
    assert dl.maybe_collect() is not None and dl.collections == 2
    # the floor is a constructor argument, an attribute and a call argument
    eng2 = _StubEngine()
    d0 = U.DeviceLeaves(eng2, auto_collect=True, floor=0)
    assert d0.auto_collect is True and d0.maybe_collect() is None  # 0 > 0 is false
    eng2.used, eng2.live = 8, 8
    assert d0.maybe_collect().kept_bytes == 8
    eng2.used = 16
    assert d0.maybe_collect() is None  # 16 == 2 * 8 + 0
    assert d0.maybe_collect(floor=0) is None
    eng2.used = 24
    assert d0.maybe_collect(floor=16) is None and d0.maybe_collect() is not None and d0.collections == 2
    # collect() passes keep and shrink on, under the lock
    held = []

    class _Lock:
        def __enter__(self):
            held.append("in")

        def __exit__(self, *a):
            held.append("out")
    d1 = U.DeviceLeaves(eng2, lock=_Lock)
    d1.collect(keep=[5, 6], shrink=True)
    keep, shrink = eng2.calls[-1]
    assert keep.tolist() == [5, 6] and keep.dtype == np.uint64 and shrink is True and held == ["in", "out"]


def test_auto_collect_runs_after_the_write_has_returned():
    """UJSONDocs calls maybe_collect() after b.write(...) of INS / RM / CLR / SET, and only with auto_collect"""
    log = []

    class _Backend:
        def write(self, cmds, identity):
            log.append("write")

        def exists(self, key):
            return True

        def elements(self, keys):
            return {}

    class _Leaves(U.LeafTable):
        auto_collect = True

        def maybe_collect(self):
            log.append("collect")
    docs = U.UJSONDocs(_Backend(), 1, _Leaves())
    docs.ins("k", ("a",), "1")
    docs.rm("k", ("a",), "1")
    docs.clr("k")
    docs.clr("k", ("a",))
    docs.set("k", ("a",), '{"b":2}')
    assert log == ["write", "collect"] * 5
    del log[:]
    docs = U.UJSONDocs(_Backend(), 1, U.LeafTable())  # the default: off
    docs.set("k", (), '{"b":2}')
    assert log == ["write"]
