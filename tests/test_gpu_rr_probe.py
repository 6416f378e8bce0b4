"""The reduced-radix layer (libff_amd/csrc/rr.cuh) on the device against the plain-integer model of tests/rr_model.py,
through Engine.rr_probe / Engine.xyzz_rr_probe, on the operand sets whose coverage tests/test_rr_model_cpu.py asserts.

Deterministic functions: the output equals the model limb for limb (and word for word, flag for flag).  Point functions:
the infinity flag is the ladder's, every coordinate of the result is the formula's residue, the exported words are the
canonical residues, and the raw limbs and the value lie inside the interval the Checker of tests/test_rr_bounds.py
derives for that state from the interval the operands were drawn from -- which ties that hand-kept mirror to the device.
No tolerances: every comparison is exact or an interval of the Checker.  One launch per case; nothing is compiled here.
"""
import functools

import numpy as np
import pytest

import rr_model as rm
import test_rr_bounds as tb

pytestmark = pytest.mark.gpu

UNIT_OPS = [(name, op) for name in rm.UNITS for op in rm.unit_ops(name)]
COORDS = ("x", "y", "zz", "zzz")


@functools.lru_cache(maxsize=None)
def _limb_case(name, op):
    """operand arrays and expected arrays of one (unit, op)"""
    u = rm.unit(name)
    s = u.s
    o = rm.limb_operands(name, op)
    args = o["args"]
    arity = len(args[0])
    if op in rm.WORD_OPS:
        arrs, w = [None] * 4, rm.word_rows(s, [a[0] for a in args])
    else:
        arrs = [rm.limb_rows([a[k] for a in args]) if k < arity else None for k in range(4)]
        w = None
    if op == "cneg":
        want = [(e, None, 0) for e in rm.cneg_expected(args)]
    else:
        want = [rm.limb_expected(name, op, a) for a in args]
    out = rm.limb_rows([e[0] for e in want])
    outw = rm.word_rows(s, [e[1] if e[1] is not None else (0,) * u.deg for e in want])
    flag = np.array([e[2] for e in want], dtype=np.uint32)
    return arrs, w, o["k"], out, outw, flag


def _run_limb(engine, name, op, arrs, w, k):
    u = rm.unit(name)
    return engine.rr_probe(u.curve, u.group, rm.ROPS[op], u.s.L, u.s.N, *arrs, w=w, k=k, rows_per_element=u.deg)


@pytest.mark.parametrize("name,op", UNIT_OPS)
def test_rr_probe(engine, name, op):
    u = rm.unit(name)
    arrs, w, k, want, want_w, want_f = _limb_case(name, op)
    out, outw, flag = _run_limb(engine, name, op, arrs, w, k)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, (name, op, "limbs differ in", int(bad.size), "rows; first element", int(bad[0]) // u.deg,
                           out[bad[0]].tolist(), want[bad[0]].tolist())
    bad = np.nonzero((outw != want_w).any(axis=1))[0]
    assert bad.size == 0, (name, op, "words differ in", int(bad.size), "rows; first element", int(bad[0]) // u.deg)
    bad = np.nonzero(flag != want_f)[0]
    assert bad.size == 0, (name, op, "flags differ in", int(bad.size), "elements; first", int(bad[0]), int(flag[bad[0]]))


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_rr_probe_launch_shapes(engine, name):
    """element counts of one lane, an odd count, exactly one wave (for a pair unit: the last pair in lanes 62 / 63), one
    pair more than a wave, exactly one block, a partial last wave behind a full block"""
    u = rm.unit(name)
    arrs, w, k, want, _, _ = _limb_case(name, "re_mul")
    wave = 64 // u.deg
    for n in (1, 63, wave, wave + 1, 256 // u.deg, 256 // u.deg + 37):
        rows = n * u.deg
        out, _, flag = _run_limb(engine, name, "re_mul", [a[:rows] if a is not None else None for a in arrs], None, k)
        assert out.shape == (rows, u.s.L) and (out == want[:rows]).all(), (name, n)
        assert not flag.any()


# ---- point level ----------------------------------------------------------------------------------------
def _pt_rows(u, cases):
    """affine words of each case -> (n * deg, 2 N) uint32: row = one component's x, y"""
    s = u.s
    x = rm.word_rows(s, [c["pt"][0] for c in cases])
    y = rm.word_rows(s, [c["pt"][1] for c in cases])
    return np.concatenate([x, y], axis=1)


def _check_result(u, i, out, outw, got_inf, want, factors, interval, tag):
    """record i of the probe's output against the wanted residues `want` (INF or one tuple per coordinate), its export
    against the canonical words, its limbs and value against the Checker's interval {coordinate: El} (or None)"""
    s = u.s
    assert bool(got_inf) == (want is rm.INF), (tag, i, "infinity flag", int(got_inf))
    ncoord = len(factors)
    words = outw[i * u.deg:(i + 1) * u.deg]
    if want is rm.INF:
        assert not words.any(), (tag, i, "export of infinity")
        return
    rec = rm.quad_of_rows(s, out, u.deg, i)
    for k in range(ncoord):
        assert u.res(rec[k], factors[k]) == want[k], (tag, i, COORDS[k], "wrong residue")
        canon = u.words_of(want[k])
        got_w = tuple(rm.words_value(words[c, k * s.N:(k + 1) * s.N]) for c in range(u.deg))
        assert got_w == canon, (tag, i, COORDS[k], "exported words")
        if interval is not None:
            for c in range(u.deg):
                msg = rm.in_interval(s, interval[k], rec[k][c])
                assert msg is None, (tag, i, COORDS[k], c, msg)


@functools.lru_cache(maxsize=None)
def _madd_intervals(name):
    """the Checker's output interval per (rung, state) of xyzz_madd_rr"""
    u = rm.unit(name)
    st, ch = rm.states(u.field, u.nr)
    lst = lambda d: [d[c] for c in COORDS]
    return {("general", "steady"): lst(tb.madd(ch, st["steady"], fq2_nr=u.nr)), ("general", "first"): lst(tb.madd(ch, st["first"], fq2_nr=u.nr)),
            "first": lst(st["first"]), "same": lst(tb.doubling_path(ch, u.nr))}


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_xyzz_madd_rr(engine, name):
    u = rm.unit(name)
    cases = rm.madd_cases(name)
    acc = rm.quad_rows([c["acc"] for c in cases], u.deg)
    fin = np.array([(1 if c["inf"] else 0) | (4 if c["neg"] else 0) for c in cases], dtype=np.uint32)
    out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS["madd"], u.s.N, acc, pt=_pt_rows(u, cases), fin=fin,
                                           rows_per_element=u.deg)
    iv = _madd_intervals(name)
    for i, c in enumerate(cases):
        tag = (name, "madd", c["rung"], c["state"])
        if c["rung"] == "point_inf":   # nothing happens: the accumulator and its flag as they were
            assert bool(fout[i] & 1) == c["inf"] and (out[i * u.deg:(i + 1) * u.deg] == acc[i * u.deg:(i + 1) * u.deg]).all(), tag
            continue
        interval = iv.get((c["rung"], c["state"]), iv.get(c["rung"]))
        _check_result(u, i, out, outw, fout[i] & 1, c["want"], ("rho", "rho", "rho_d", "rho_d"), interval, tag)


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_xyzz_rr_first(engine, name):
    """xyzz_rr_first limb for limb: the coordinates' first-point form (reduced where the unit needs it), -y carried once,
    zz = zzz = 2^(B L + D) mod p"""
    u = rm.unit(name)
    s = u.s
    nr = u.nr if u.deg == 2 else 0
    ws = rm.first_words(u.field)
    n = 255
    pts = [(tuple(ws[(3 * i + c) % len(ws)] for c in range(u.deg)), tuple(ws[(5 * i + 7 * c + 1) % len(ws)] for c in range(u.deg)))
           for i in range(n)]
    cases = [dict(pt=p) for p in pts]
    fin = np.array([4 * (i % 2) for i in range(n)], dtype=np.uint32)
    acc = np.zeros((n * u.deg, 4 * s.L), dtype=np.int32)
    out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS["first"], s.N, acc, pt=_pt_rows(u, cases), fin=fin,
                                           rows_per_element=u.deg)
    st, _ = rm.states(u.field, u.nr)
    one = rm._one_el(u, s.BL + s.D)
    for i, (wx, wy) in enumerate(pts):
        x = [rm.first_coord(s, nr, w) for w in wx]
        if s.first_needs_reduction(nr):
            x = [rm.norm(s, c) for c in x]
        y = [rm.norm(s, [-l if i % 2 else l for l in rm.first_coord(s, nr, w)]) for w in wy]
        rec = rm.quad_of_rows(s, out, u.deg, i)
        assert rec == [x, y, one, one], (name, i)
        assert not fout[i]
        want = (u.res_words(wx), u.F.sub(u.F.zero, u.res_words(wy)) if i % 2 else u.res_words(wy), u.F.one, u.F.one)
        _check_result(u, i, out, outw, 0, want, ("rho", "rho", "rho_d", "rho_d"), [st["first"][c] for c in COORDS], (name, "first"))


@pytest.mark.parametrize("op", ["rec_to_rho", "export", "export_rho"])
@pytest.mark.parametrize("name", list(rm.UNITS))
def test_xyzz_rr_conversions(engine, name, op):
    """xyzz_rec_to_rho limb for limb (zz, zzz times 2^(32 N) / rho, x and y untouched) and the export of a record in both
    forms, on the accumulators of the mixed-addition cases"""
    u = rm.unit(name)
    s = u.s
    cases = [c for c in rm.madd_cases(name) if not c["inf"]]
    acc = rm.quad_rows([c["acc"] for c in cases], u.deg)
    out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS[op], s.N, acc, rows_per_element=u.deg)
    st, ch = rm.states(u.field, u.nr)
    assert not fout.any()
    for i, c in enumerate(cases):
        rec = rm.quad_of_rows(s, out, u.deg, i)
        zfac = "rho" if op == "export_rho" else "rho_d"
        want = tuple(u.res(c["acc"][k], "rho" if k < 2 else zfac) for k in range(4))
        interval = None
        if op == "rec_to_rho":
            model = c["acc"][:2] + [[rm.mul_pow2(s, comp, 32 * s.N) for comp in c["acc"][k]] for k in (2, 3)]
            assert rec == model, (name, op, i)
            interval = [tb.rec_to_rho(ch, st[c["state"]])[k] for k in COORDS]
        else:
            assert rec == c["acc"], (name, op, i)
        _check_result(u, i, out, outw, 0, want, ("rho", "rho", "rho" if op != "export" else "rho_d", "rho" if op != "export" else "rho_d"),
                      interval, (name, op, c["state"]))


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_xyzz_dbl_rho(engine, name):
    u = rm.unit(name)
    cases = rm.dbl_cases(name)
    acc = rm.quad_rows([c["a"] for c in cases], u.deg)
    fin = np.array([1 if c["inf"] else 0 for c in cases], dtype=np.uint32)
    out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS["dbl_rho"], u.s.N, acc, fin=fin, rows_per_element=u.deg)
    st, ch = rm.states(u.field, u.nr)
    for i, c in enumerate(cases):
        interval = [tb.dbl_rho(ch, st[c["state"]], u.nr)[k] for k in COORDS] if c["rung"] == "double" else None
        _check_result(u, i, out, outw, fout[i] & 1, c["want"], ("rho",) * 4, interval, (name, "dbl_rho", c["rung"], c["state"]))


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_xyzz_add_rho(engine, name):
    u = rm.unit(name)
    cases = rm.add_cases(name)
    a = rm.quad_rows([c["a"] for c in cases], u.deg)
    b = rm.quad_rows([c["b"] for c in cases], u.deg)
    fin = np.array([(1 if c["a_inf"] else 0) | (2 if c["b_inf"] else 0) for c in cases], dtype=np.uint32)
    out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS["add_rho"], u.s.N, a, sec=b, fin=fin, rows_per_element=u.deg)
    st, ch = rm.states(u.field, u.nr)
    for i, c in enumerate(cases):
        tag = (name, "add_rho", c["rung"], c["sa"], c["sb"])
        rows = slice(i * u.deg, (i + 1) * u.deg)
        if c["rung"] == "b_inf":
            assert bool(fout[i] & 1) == c["a_inf"] and (out[rows] == a[rows]).all(), tag
            continue
        if c["rung"] == "a_inf":
            assert not fout[i] & 1 and (out[rows] == b[rows]).all(), tag
        interval = None
        if c["rung"] == "general":
            interval = [tb.add_rho(ch, st[c["sa"]], st[c["sb"]], u.nr)[k] for k in COORDS]
        elif c["rung"] == "equal":
            interval = [tb.dbl_rho(ch, st[c["sa"]], u.nr)[k] for k in COORDS]
        _check_result(u, i, out, outw, fout[i] & 1, c["want"], ("rho",) * 4, interval, tag)


@pytest.mark.parametrize("name", list(rm.UNITS))
def test_jac_rr(engine, name):
    """jac_dbl_rr, jac_madd_rr and jac_is_inf_rr: one launch each"""
    u = rm.unit(name)
    s = u.s
    ch = tb.Checker(s)
    px, py, one = tb.jac_operands(ch)
    state = (px, py, px)   # Z of a running point is a product's output too
    iv = {("dbl", "double"): tb.jac_dbl(ch, state), ("madd", "general"): tb.jac_madd(ch, state, px, py),
          ("madd", "same"): tb.jac_dbl(ch, (px, py, one))}
    zero = [[0] * s.L for _ in range(u.deg)]
    for op in ("dbl", "madd", "is_inf"):
        cases = [c for c in rm.jac_cases(name) if c["op"] == op]
        acc = rm.quad_rows([c["a"] + [zero] for c in cases], u.deg)
        sec = rm.quad_rows([(c["q"] + [zero, zero]) for c in cases], u.deg) if op == "madd" else None
        fin = np.array([1 if c["inf"] else 0 for c in cases], dtype=np.uint32)
        out, outw, fout = engine.xyzz_rr_probe(u.curve, u.group, rm.XOPS["jac_" + op], s.N, acc, sec=sec, fin=fin,
                                               rows_per_element=u.deg)
        for i, c in enumerate(cases):
            tag = (name, "jac_" + op, c["rung"])
            if op == "is_inf":
                assert bool(fout[i] & 2) == c["want"], tag
                continue
            interval = iv.get((op, c["rung"]))
            if c["rung"] == "first":   # the affine point as it came, Z = one
                rec = rm.quad_of_rows(s, out, u.deg, i)
                assert rec[:3] == c["q"] + [rm._one_el(u, s.BL)], tag
            _check_result(u, i, out, outw, fout[i] & 1, c["want"], ("rho",) * 3, interval, tag)


@pytest.mark.parametrize("name", ["mnt4_g1", "mnt4_g2", "mnt6_g1"])
def test_rr_probe_unsupported_on_mnt(engine, name):
    """the MNT units do not carry the layer: AMDMSM_ERR_UNSUPPORTED, a message naming the group, the output untouched"""
    import ctypes

    import field_model as fm
    import libff_amd

    _, curve, group, _, _, _ = fm.GROUP_BY_NAME[name]
    a = np.full((8, 16), 7, dtype=np.int32)
    sentinel = np.full((8, 64), 0x5a5a5a5a, dtype=np.uint32)
    ptrs = engine._dev_arrays(a, sentinel, sentinel, sentinel)
    try:
        for entry, call in (("amdmsm_rr_probe_device", lambda: engine.lib.amdmsm_rr_probe_device(
                engine.h, curve, group, 0, 0, ptrs[0], ptrs[0], None, None, None, ptrs[1], ptrs[2], ptrs[3], ctypes.c_size_t(8))),
                            ("amdmsm_xyzz_rr_probe_device", lambda: engine.lib.amdmsm_xyzz_rr_probe_device(
                                engine.h, curve, group, 3, ptrs[0], None, None, None, ptrs[1], ptrs[2], ptrs[3], ctypes.c_size_t(2)))):
            assert call() == -3, entry   # AMDMSM_ERR_UNSUPPORTED
            assert name in engine.lib.amdmsm_last_error(engine.h).decode(), entry
            for p in ptrs[1:]:
                back = np.zeros_like(sentinel)
                engine.d2h(back, p)
                assert (back == sentinel).all(), (entry, "output written")
        with pytest.raises(libff_amd.engine.AmdMsmError) as e:
            engine.rr_probe(curve, group, 0, 16, 10, a=a, b=a)
        assert e.value.code == -3 and name in str(e.value)
    finally:
        for p in ptrs:
            engine.free(p)
