"""What the tests of Engine.group_matrix_apply share: the sparse matrix times point vector

    out[i] = sum over the entries k of row i of  coeff[k] * P[col[k]]

with every input point a known multiple a_c G of the generator (group_fft_model.group_of(port, name).records), so that
row i is ((sum coeff * a_col) mod r) G by fr_matrix_model.apply -- Python integers and the scalar multiples of the
oracle, nothing of the library.  Records are compared bit for bit in special form.  Nothing here knows how the library
stores a matrix, ranks its general entries or folds a wave."""
import contextlib
import os
import random

import numpy as np

import fr_matrix_model as mm
import group_fft_model as gm
from fr_matrix_model import Csr  # noqa: F401

ALL_NAMES = gm.ALL_NAMES
# the thresholds the small matrices are loaded with: rows of 4 entries take a wave, rows above 64 are split
SMALL = {"AMDMSM_FR_MATRIX_WAVE_ROW": "4", "AMDMSM_FR_MATRIX_SPLIT_ROW": "64"}
SMALL_LENGTHS = [0, 1, 2, 3] * 17 + [4, 5, 63, 64, 65, 128, 130]   # 68 lane rows: a second, partly empty lane block
SMALL_POINTS = 24


@contextlib.contextmanager
def env(values):
    """the environment of a block (the load reads it per call), as it was afterwards"""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def field_of(g):
    return mm.field(g.curve)


def load(engine, g, m, transposed=False, small=True):
    """the handle of m, or of its transpose, of g's curve"""
    off, cols, co = m.arrays(field_of(g), True)
    fn = engine.fr_matrix_load_transposed if transposed else engine.fr_matrix_load
    with env(SMALL if small else {}):
        return fn(g.curve, off, cols, co, m.n_cols, plain=True)


def transpose(m):
    """the CSR of the transpose: row c holds (i, coeff) for every entry (i, c) of m, in ascending i"""
    rows = [[] for _ in range(m.n_cols)]
    for i, row in enumerate(m.rows):
        for c, v in row:
            rows[c].append((i, v))
    return mm.Csr(rows, m.n_rows)


def expected(g, m, logs):
    """the rows as special-form records"""
    return g.records(mm.apply(m, logs, g.r))


def special(g, got, out_form):
    from libff_amd import OUT_AFFINE

    return got if out_form == OUT_AFFINE or len(got) == 0 else g.special(got)


def small_matrix(g, seed, max_general=None, zeros=True):
    """rows of every job kind over SMALL_POINTS points: coefficients from pick_coeff without zeros, a few zero entries in
    rows of their own; max_general: at most that many coefficients other than 1 and r - 1 (the rest become +-1)"""
    m = mm.random_matrix(g.r, SMALL_LENGTHS, SMALL_POINTS, seed)
    rows = [list(row) for row in m.rows]
    if max_general is not None:
        rng, seen = random.Random(seed + 1), 0
        for row in rows:
            for k, (c, v) in enumerate(row):
                if v not in (1, g.r - 1):
                    seen += 1
                    if seen > max_general:
                        row[k] = (c, rng.choice((1, g.r - 1)))
    if zeros:
        rows += [[(3, 0)], [(5, 0), (7, 0)], [(1, 0), (2, 1), (9, 0)]]
    return mm.Csr(rows, SMALL_POINTS)


def small_logs(g, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, g.r) for _ in range(SMALL_POINTS)]


_cases = {}


def small_case(port, name, seed=5):
    """(group, matrix, logs, points, expected rows) of the small matrix of a group: computed once, shared, never changed"""
    key = (name, seed)
    if key not in _cases:
        g = gm.group_of(port, name)
        m = small_matrix(g, seed, max_general=40 if name.startswith("bw6_761") else None)
        logs = small_logs(g, seed)
        pts, want = g.records(logs), expected(g, m, logs)
        pts.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (g, m, logs, pts, want)
    return _cases[key]


def degenerate_matrix(g):
    """rows whose additions meet the equal point, the opposite point and infinity, over the logs DEGENERATE_LOGS(r)"""
    r, gen = g.r, 0x1234567
    lanes = [[(0, 1), (1, 1)], [(0, 1), (5, 1)], [(4, 1)], [(4, gen)], [(0, 1), (1, 1), (2, 1)],
             [(0, 1), (1, 1), (6, 1), (3, 1)], [(2, 1), (0, 2)], [(2, 1), (0, r - 2)]]
    waves = [[(0, 1)] * 64, [(0, 1)] * 32 + [(0, r - 1)] * 32]
    splits = [[(0, 1)] * 128, [(0, 1)] * 64 + [(0, r - 1)] * 64]
    return mm.Csr(lanes + waves + splits, 8)


def degenerate_logs(g):
    r = g.r
    return [1, 1, 2, 3, 0, r - 1, r - 2, 5]
