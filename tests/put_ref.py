"""Numpy / plain-Python restatements of what the keyed writes (k_put.hip)
compute, for the tests: the (pre, lr) value handles of jy_values_pack_mem, the
cut of a TLOG batch into units and rounds, and a small model of the TLOG write
commands (repo_tlog.pony:85-111) to apply a batch either one command at a time
or round by round."""
import numpy as np

LR_LEN_BITS = 24
INS, TRIMAT, TRIM, CLR = 0, 1, 2, 3
UNIT_MAX = 64


def pack_ref(values, arena_len):
    """(pre u64[n], lr u64[n], arena bytes appended from arena_len on)"""
    lens = np.array([len(v) for v in values], np.uint64)
    long_ = lens > 8
    padded = np.where(long_, (lens + np.uint64(7)) & ~np.uint64(7), np.uint64(0))
    base = (arena_len + 7) & ~7
    at = np.uint64(base) + np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.uint64) if len(values) else lens
    pre = np.zeros(len(values), np.uint64)
    for i, v in enumerate(values):
        pre[i] = int.from_bytes(bytes(v[:8]).ljust(8, b"\0"), "big")
    lr = np.where(long_, (at << np.uint64(LR_LEN_BITS)) | lens, lens).astype(np.uint64)
    tail = bytearray(base - arena_len)
    for v, p, l in zip(values, padded, long_):
        if l:
            tail += bytes(v).ljust(int(p), b"\0")
    return pre, lr, bytes(tail)


def units_ref(ops, slots, unit_max=UNIT_MAX):
    """-> [(round, slot, [command indices])] in the order the device lists them
    (by round, then by slot): commands grouped by slot in call order, each
    slot's run cut into units (up to unit_max consecutive INS, or one other
    command), the j-th unit of a slot in round j.  The stable sort by slot,
    the stretch starts and the unit ids are computed as the kernels do."""
    ops, slots = np.asarray(ops), np.asarray(slots)
    n = len(ops)
    order = np.argsort(slots, kind="stable")
    so, ss = ops[order], slots[order]
    head = np.ones(n, bool)
    head[1:] = ss[1:] != ss[:-1]
    start = head.copy()
    start[1:] |= (so[1:] != INS) | (so[:-1] != INS)
    sst = np.maximum.accumulate(np.where(start, np.arange(n) + 1, 0))  # stretch start + 1
    ustart = (np.arange(n) + 1 - sst) % unit_max == 0
    uid = np.cumsum(ustart)  # 1-based
    huid = np.maximum.accumulate(np.where(head, uid, 0))
    rnd = uid - huid
    units = []
    for p in np.nonzero(ustart)[0]:
        q = p + 1
        while q < n and not ustart[q]:
            q += 1
        units.append((int(rnd[p]), int(ss[p]), [int(i) for i in order[p:q]]))
    units.sort(key=lambda u: (u[0], u[1]))
    return units


class TLogModel:
    """one log and its pending delta, as the reference's TLog and RepoTLOG keep them"""

    def __init__(self):
        self.cut, self.ents = 0, set()
        self.dcut, self.dents, self.pending = 0, set(), False

    def _raise(self, c):
        if c <= self.cut:
            return False
        self.cut = c
        self.ents = {e for e in self.ents if e[0] >= c}
        return True

    def _delta_raise(self, c):
        if c > self.dcut:
            self.dcut = c
            self.dents = {e for e in self.dents if e[0] >= c}

    def _judge(self, cmd):
        """-> (entry or None, raise or 0, changed) against the state as it is"""
        op = cmd[0]
        if op == INS:
            e = (cmd[1], cmd[2])
            return e, 0, e[0] >= self.cut and e not in self.ents
        if op == TRIMAT:
            return None, cmd[1], cmd[1] > self.cut
        count = 0 if op == CLR else cmd[1]
        order = sorted(self.ents, reverse=True)
        if count == 0:
            c = order[0][0] + 1 if order else 0
        else:
            c = order[count - 1][0] if count - 1 < len(order) else 0
        return None, c, c > self.cut

    def apply_unit(self, cmds):
        """a unit: every command judged against the state before the unit
        (duplicates inside it dropped), then the state and the delta merged"""
        self.pending = True
        seen, judged = set(), []
        for c in cmds:
            if c[0] == INS and (c[1], c[2]) in seen:
                continue
            if c[0] == INS:
                seen.add((c[1], c[2]))
            judged.append(self._judge(c))
        for e, c, changed in judged:
            if e is not None:
                if e[0] >= self.cut:
                    self.ents.add(e)
                if changed and e[0] >= self.dcut:
                    self.dents.add(e)
            elif changed:
                self._raise(c)
                self._delta_raise(c)

    def snapshot(self):
        return (self.cut, frozenset(self.ents), self.dcut, frozenset(self.dents), self.pending)


def apply_in_order(cmds, slots):
    logs = {}
    for c, s in zip(cmds, slots):
        logs.setdefault(s, TLogModel()).apply_unit([c])
    return {s: l.snapshot() for s, l in logs.items()}


def apply_in_rounds(cmds, slots, unit_max=UNIT_MAX):
    logs = {}
    rounds = 0
    for rnd, s, idx in units_ref([c[0] for c in cmds], slots, unit_max):
        rounds = max(rounds, rnd + 1)
        logs.setdefault(s, TLogModel()).apply_unit([cmds[i] for i in idx])
    return {s: l.snapshot() for s, l in logs.items()}, rounds
