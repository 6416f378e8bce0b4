"""Expected values and inputs of the segmented-MSM tests (tests/test_gpu_segments.py).

The groups, their 257-element vector (points, scalars, the products k_i * P_i) and the way records are made come from
tests/test_gpu_scalar_mul_vec.py -- computed once per group and shared with those tests.  A segment's expected sum is the
group sum of its terms' products: oracle.port additions for the eight pairing-curve groups, tests/mnt_model.py additions
for the three MNT groups.  Nothing here calls the engine."""
import numpy as np

import mnt_model as mm
from test_gpu_scalar_mul_vec import ALL, EDGE_SMALL, MntGroup, _hip_runtime, group_of, vector  # noqa: F401

SIZE_MAX = 2 ** 64 - 1
# segment lengths of the 65-segment case: every length of {0, 1, 2, 3, 63, 64, 65, 257}, empty segments first, last and
# next to each other, one chain of 257 terms among short ones
LENS_65 = ([0, 0, 1, 2, 3, 63, 64, 65, 257, 0, 0, 3, 2, 1] + [1, 2, 3, 0, 64, 63, 65, 1] * 6 + [2, 0, 0])
assert len(LENS_65) == 65
# the short mixture the form, routing and chunking tests share
LENS_SMALL = [0, 1, 2, 3, 63, 0, 65, 64, 257, 0]


def offsets_of(lens, first=0):
    return np.cumsum([first] + list(lens)).astype(np.uint64)


class Sums:
    """group sums of product records for one group"""

    def __init__(self, g, port):
        self.g, self.port = g, port
        self.mnt = isinstance(g, MntGroup)

    def segments(self, prods, offsets, column=None):
        """special-form records of sum(prods[column(j, i)]) over the terms i of segment j; column defaults to the term"""
        g, out = self.g, []
        if self.mnt:
            pts = [g.model.point(r) for r in prods]
        for j in range(len(offsets) - 1):
            lo, hi = int(offsets[j]), int(offsets[j + 1])
            idx = [i if column is None else column(j, i) for i in range(lo, hi)]
            if self.mnt:
                acc = mm.INF
                for i in idx:
                    acc = g.model.add(acc, pts[i])
                out.append(acc)
            else:
                acc = g.infinity()
                for i in idx:
                    acc = self.port.group_op(g.curve, g.group, 0, acc, prods[i])
                out.append(self.port.group_op(g.curve, g.group, 4, acc))
        if not out:
            return np.zeros((0, g.gl), dtype=np.uint64)
        return g.model.records(out) if self.mnt else np.stack(out)


_cases = {}


def cycled(port, name, n_terms):
    """(group, points, scalars as integers, products) of n_terms terms that cycle through the group's vector"""
    g, recs, ks, want = vector(port, name)
    idx = np.arange(n_terms) % len(recs)
    return g, recs[idx], [ks[i] for i in idx], want[idx]


def case(port, name, lens, first, slack):
    """One unshared input and its expected sums, computed once and left unchanged: segments of the given lengths over
    cycled terms, `first` terms in front of the first segment and `slack` behind the last one."""
    key = (name, tuple(lens), first, slack)
    if key not in _cases:
        offs = offsets_of(lens, first)
        g, recs, ks, prods = cycled(port, name, int(offs[-1]) + slack)
        want = Sums(g, port).segments(prods, offs)
        for a in (offs, want):
            a.setflags(write=False)
        _cases[key] = (g, recs, ks, offs, want)
    return _cases[key]
