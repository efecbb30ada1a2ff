"""Anti-entropy between two nodes by bucketed state digests.

Each side computes its [nbuckets, 4] digest of one type (Node.digest;
jy_*_state_digest), the rows are compared, and only the keys of the buckets
that differ are dumped (Node.repair_batches) and converged into the other
side (Node.restore), both ways.  The join is a semilattice, so after one
exchange both sides hold the join of the two states and the digests agree.
"""
import numpy as np


def diff(mine, theirs):
    """the indices of the buckets whose 4-word rows differ (ascending, int64)"""
    a, b = np.asarray(mine, np.uint64), np.asarray(theirs, np.uint64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"digests must both be [nbuckets, 4]: {a.shape} and {b.shape}")
    return np.nonzero((a != b).any(axis=1))[0]


def sync(a, b, ctype, nbuckets=1024, max_keys=65536, leaves=False):
    """make nodes a and b hold the same state of one type, shipping only the
    buckets whose digests differ: a -> b and b -> a per round, columns mapped
    through the sender's replica_ids().  Returns {rounds, buckets, keys_sent};
    one round suffices (asserted: a second round that still leaves the digests
    different raises).  leaves=True: UJSON repair batches carry their leaves, so
    the receiver's leaf store can render what it was sent."""
    kw = {"leaves": True} if leaves else {}
    rounds, nbad, sent = 0, 0, 0
    while True:
        da, db = a.digest(ctype, nbuckets, max_keys), b.digest(ctype, nbuckets, max_keys)
        bad = diff(da, db)
        if len(bad) == 0:
            return {"rounds": rounds, "buckets": nbad, "keys_sent": sent}
        if rounds == 2:
            raise RuntimeError(f"digests still differ in {len(bad)} buckets after two rounds")
        rounds += 1
        if rounds == 1:
            nbad = len(bad)
        out = []  # both sides are dumped before either is changed
        for src, dst in ((a, b), (b, a)):
            batches = [w for _, w in src.repair_batches(ctype, nbuckets, bad, max_keys, **kw)]
            sent += sum(len(w["key_offs"]) - 1 for w in batches)
            out.append((dst, batches, src.replica_ids()))
        for dst, batches, ids in out:
            dst.restore(ctype, batches, col_ids=ids)
        a.sync()
        b.sync()
