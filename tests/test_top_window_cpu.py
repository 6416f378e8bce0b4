"""The bound on the top window's bucket index that the bucket sort cuts its bins by (group_vtable.h top_window_bits, read
through amdmsm_plan_top_window), checked without a device on Python big integers: for every group and every window
size the planner can be given, with the split and without it, no scalar of the set produces a top-window index of tb
bits or more -- and some scalar of the set comes within one bit of it, so the shift the sort derives is not silently
zero.  The set: 0, 1, r - 1, (r - 1) / 2, the scalars that maximise |k1| and |k2| of the split, 2^14 random scalars.
Plain scalars (amdmsm_opts.scalars_plain) need not be below r: there the set is every one of these, 2^(32 fr_words) - 1 and
- 2, and random integers of the full word length -- the split's bound must hold for their halves too, and without the
split only the word length bounds the top window."""
import numpy as np
import pytest

import libff_amd
import mnt_model as mm
import top_window as tw
from common import GROUPS

ALL = [(name, curve, group) for name, curve, group in GROUPS] + [("mnt4_g1", libff_amd.MNT4, 1), ("mnt4_g2", libff_amd.MNT4, 2),
                                                                 ("mnt6_g1", libff_amd.MNT6, 1)]
_sets = {}


def scalar_set(curve):
    """(r, plain scalars, their split halves as magnitudes or None where the curve has no split)"""
    if curve not in _sets:
        gp_mod = tw.gen_params()
        cname = tw.CURVE_NAMES[curve]
        if cname in gp_mod.CURVES:
            r = gp_mod.CURVES[cname]["r"]
            gp = gp_mod.glv_params(cname)
            extra = list(tw.split_maximisers(cname))
        else:
            r, gp, extra = (mm.MNT4 if curve == libff_amd.MNT4 else mm.MNT6).r, None, []
        rng = np.random.default_rng(1000 + curve)
        nbytes = (r.bit_length() + 7) // 8 + 8
        ks = [0, 1, r - 1, (r - 1) // 2] + extra + [int.from_bytes(rng.bytes(nbytes), "little") % r for _ in range(1 << 14)]
        bits = libff_amd.sizes(curve, 1)["fr_bytes"] * 8
        wide = [(1 << bits) - 1, (1 << bits) - 2, 1 << (bits - 1)] + [int.from_bytes(rng.bytes(bits // 8), "little") for _ in range(1 << 12)]
        halves = None
        if gp is not None:
            halves = [abs(h) for k in ks + wide for h in gp_mod.glv_split(gp, k)]
            assert max(halves) <= gp["bound"]
        _sets[curve] = (r, ks, halves, ks + wide)
    return _sets[curve]


def test_top_digit_model():
    """the one-step top digit equals the digit-by-digit recoding"""
    rng = np.random.default_rng(3)
    for _ in range(3000):
        c, W = int(rng.integers(2, 23)), int(rng.integers(1, 24))
        m = int.from_bytes(rng.bytes(64), "little") & ((1 << max(0, c * W - 2)) - 1)   # what the planned windows cover
        assert tw.signed_digits(m, c, W)[-1] == tw.top_digit(m, c, W)


@pytest.mark.parametrize("mode", ["mont", "split", "plain_words"])
@pytest.mark.parametrize("name,curve,group", ALL)
def test_plan_bound_holds_and_is_tight(name, curve, group, mode):
    """mont: Montgomery scalars, no split; split: either form, split; plain_words: scalars_plain, no split"""
    r, ks, halves, wide = scalar_set(curve)
    split, plain = mode == "split", mode == "plain_words"
    if split and halves is None:
        # MNT4 / MNT6: amdmsm_opts.endomorphism is ignored, the plan is the plain one
        assert not libff_amd.plan(curve, group, 1000, endomorphism=2)["endomorphism"]
        halves = ks
    values = halves if split else wide if plain else ks
    shifts = 0
    for c in range(2, 23):
        for n in (1000, 1 << 20):
            t = tw.plan_top_window(curve, group, n, window_bits=c, endomorphism=2 if split else -1, scalars_plain=plain)
            p = libff_amd.plan(curve, group, n, window_bits=c, endomorphism=2 if split else -1)
            if p["endomorphism"]:   # the halves obey the same bound whichever form the scalars come in
                assert t == tw.plan_top_window(curve, group, n, window_bits=c, endomorphism=2, scalars_plain=True)
            geo = libff_amd.plan_sort(curve, group, n, window_bits=c, endomorphism=2 if split else -1)
            assert (t["c"], t["num_windows"]) == (c, p["num_windows"])
            assert 0 <= t["tb"] <= c - 1
            want_shift = min(geo["fine_bits"], c - 1 - t["tb"]) if p["num_windows"] > 1 else 0
            assert t["shift"] == want_shift, (c, n, t, geo)
            shifts += t["shift"]
        W, tb = t["num_windows"], t["tb"]
        # (a zero top digit makes no entry)
        assert tw.max_top_index_bits(values[:64], c, W) == max(tw.top_index_bits(m, c, W) or 0 for m in values[:64])
        assert tb - 1 <= tw.max_top_index_bits(values, c, W) <= tb, (c, W, tb)
    # (without the split, plain scalars of the full word length leave a spare bit only where the windows overshoot it)
    assert shifts > 0 or plain
