"""Integer model of the scans and of the batch inversion over Fr that Engine.fr_scan and Engine.fr_batch_invert compute,

    forward:  y_(-1) = init,  y_i = a_i y_(i-1) + b_i,  i = 0 .. n - 1,   total = y_(n-1)
    reverse:  y_n    = init,  y_i = a_i y_(i+1) + b_i,  i = n - 1 .. 0,   total = y_0
    out[i] = y_i (inclusive) or the value that enters record i (exclusive);   1 / x as x^(r - 2), 1 / 0 = 0,

for the tests of those entries: the recurrence as a loop, the inversion as a power, the arithmetic the plan entry
reports, and the two record forms (fr_fft_model.Field).  Python integers only.  Nothing here knows of lanes, of the
order in which the library composes the maps, or of Montgomery's trick."""
from fr_fft_model import CURVES, field, random_vector  # noqa: F401

LANES = 256        # lanes of a workgroup: a tile is LANES * per_lane records
MAX_N = 1 << 28


def scan(r, n, a=None, b=None, a_const=None, init=None, reverse=False, exclusive=False):
    """(out, total).  a, b: lists or None; a_const: an int or None; init None: 1 without b, 0 with it"""
    assert a is None or a_const is None
    assert a is not None or a_const is not None or b is not None
    y = (0 if b is not None else 1) if init is None else init % r
    out = [0] * n
    order = range(n - 1, -1, -1) if reverse else range(n)
    for i in order:
        ai = a[i] if a is not None else (a_const if a_const is not None else 1)
        bi = b[i] if b is not None else 0
        before = y
        y = (ai * y + bi) % r
        out[i] = before if exclusive else y
    return out, y


_inverses = {}


def invert(r, values):
    """(out, zero_count); the power is taken once per distinct value"""
    out = []
    for v in values:
        if (r, v) not in _inverses:
            _inverses[(r, v)] = pow(v, r - 2, r) if v % r else 0
        out.append(_inverses[(r, v)])
    return out, sum(1 for v in values if v % r == 0)


def inverse(r, x):
    return pow(x, r - 2, r)


def plan(n, tile_log2, rec_bytes, a=True, b=False, invert=False):
    """what amdmsm_plan_fr_scan reports for the tiled path, from the tile alone"""
    tile = 1 << tile_log2
    tiles = (n + tile - 1) // tile
    align = lambda x: (x + 255) // 256 * 256
    vec = align(max(tiles, 1) * rec_bytes)
    fold = (1 if a else 0) + (1 if a and b else 0)
    g = 1   # tiles to a lane of the spine: enough to bring them into 64 lanes' reach, at most 1, 4, 16 by the tile
    while g < 1 << (2 * (tile_log2 - 8)) and 64 * g < tiles:
        g *= 2
    return {"tile": tile, "per_lane": tile // LANES, "spine_step": LANES * g, "launches": 3 if n else 1,
            "workspace_bytes": 3 * vec + align(max(tiles, 1) * 4),
            "products_per_record": 4 if invert else 2 * fold + (1 if a else 0)}


def synthetic_division_holds(r, p, z, q, total):
    """p(X) - p(z) = (X - z) q(X), coefficient by coefficient; total = p(z)"""
    n = len(p)
    pz = 0
    for c in reversed(p):
        pz = (pz * z + c) % r
    if total != pz or (n and q[n - 1] != 0):
        return False
    # (X - z) q(X): coefficient i is q[i - 1] - z q[i]
    for i in range(n):
        want = (p[i] - (pz if i == 0 else 0)) % r
        got = ((q[i - 1] if i else 0) - z * q[i]) % r
        if want != got:
            return False
    return True
