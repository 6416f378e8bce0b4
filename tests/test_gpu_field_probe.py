"""The 32-bit-limb field layer (fp.cuh, fp2.cuh) and the extended-Jacobian point functions of ec.cuh on the device,
in both element types -- the cold one (impl 0) and the fully inlined one (impl 1) -- against the plain-integer model
of tests/field_model.py, on the operand sets whose branch coverage tests/test_field_model_cpu.py asserts.

Canonical ops: the output equals the model word for word (sqrt: the flag says whether a is a square, and out^2 == a
where it is).  Almost-reduced ops: every component of the output is below 2p and congruent to the exact value
(canon: the canonical representative, word for word; is_zero_lz: the flag).  One launch per case.
"""
import functools

import numpy as np
import pytest

import field_model as fm

pytestmark = pytest.mark.gpu

NAMES = [g[0] for g in fm.GROUPS]


@functools.lru_cache(maxsize=None)
def _arrays(name, op):
    """operand word arrays and, for the word-for-word ops, the expected words (shared by both impls)"""
    E = fm.ext(name)
    args = fm.operands(name, op)
    arrs = [fm.to_words(E.F, [a[k] for a in args]) for k in range(len(args[0]))]
    want = None
    if op in fm.CANONICAL_OPS and op != "sqrt" or op == "canon":
        want = fm.to_words(E.F, [fm.exact(E, op, a) for a in args])
    return arrs, want


@functools.lru_cache(maxsize=None)
def _lazy_want(name, op):
    """exact residues of the almost-reduced value ops, computed once for both impls"""
    E = fm.ext(name)
    return [fm.exact(E, op, a) for a in fm.operands(name, op)]


@pytest.mark.parametrize("op", list(fm.OPS))
@pytest.mark.parametrize("impl", [0, 1], ids=["E", "EI"])
@pytest.mark.parametrize("name", NAMES)
def test_field_probe(engine, name, impl, op):
    _, curve, group, _, deg, _ = fm.GROUP_BY_NAME[name]
    E = fm.ext(name)
    arrs, want = _arrays(name, op)
    out, flag = engine.field_probe(curve, group, impl, fm.OPS[op], *arrs)
    if want is not None:
        bad = np.nonzero((out != want).any(axis=1))[0]
        assert bad.size == 0, (name, impl, op, int(bad.size), [hex(c) for c in fm.operands(name, op)[int(bad[0])][0]])
        assert not flag.any()
        return
    args = fm.operands(name, op)
    outs = fm.from_words(E.F, out, deg)
    if op in ("sqrt", "is_zero_lz"):
        bad = [(i, msg) for i, (a, o, f) in enumerate(zip(args, outs, flag)) for msg in [fm.check(E, op, a, o, int(f))] if msg]
    else:   # out < 2p per component and out mod p exact (fm.check, with the exact values shared)
        p, p2 = E.F.p, 2 * E.F.p
        bad = [(i, "not below 2p" if max(o) >= p2 else "wrong residue") for i, (o, w) in enumerate(zip(outs, _lazy_want(name, op)))
               if max(o) >= p2 or tuple(c % p for c in o) != w]
        assert not flag.any()
    assert not bad, (name, impl, op, len(bad), bad[0][1], [[hex(c) for c in e] for e in args[bad[0][0]]])


@pytest.mark.parametrize("op", list(fm.XOPS))
@pytest.mark.parametrize("impl", [0, 1], ids=["E", "EI"])
@pytest.mark.parametrize("name", NAMES)
def test_xyzz_probe(engine, name, impl, op):
    """xyzz_madd_lz, xyzz_madd, xyzz_add, xyzz_dbl, xyzz_dbl_affine and xyzz_to_jac in affine form against the curve
    model: general, equal, opposite and infinite operands; the almost-reduced addition on every representative"""
    _, curve, group, _, deg, _ = fm.GROUP_BY_NAME[name]
    C = fm.curve(name)
    E, p = C.E, C.E.F.p
    acc, sec, want = fm.point_cases(name, op)
    flat = lambda recs: np.concatenate([fm.to_words(E.F, [r[k] for r in recs]) for k in range(len(recs[0]))], axis=1)
    out = engine.xyzz_probe(curve, group, impl, fm.XOPS[op], flat(acc), None if sec is None else flat(sec))
    cw = out.shape[1] // 4
    comps = [fm.from_words(E.F, out[:, k * cw:(k + 1) * cw], deg) for k in range(4)]
    bound = 2 * p if op == "madd_lz" else p
    for i, w in enumerate(want):
        rec = tuple(comps[k][i] for k in range(4))
        assert all(c < bound for e in rec for c in e), (name, impl, op, i, "component out of range")
        got = C.of_jac(rec) if op == "to_jac" else C.of_xyzz(rec)
        assert got == w, (name, impl, op, i)
