"""MNT4-298 G1 / G2 and MNT6-298 G1 on the device (curve ids 4 and 5): field and group primitives, multi_exp in every base form,
method and output form, the a != 0 doubling inside the bucket accumulation (equal and opposite bases in one bucket),
awkward window sizes, filter_one_zero, batch_exp, batch_to_special, batches, registered bases, several contexts and
closed forms at 2^16 / 2^20 -- all checked against the pure-integer model (tests/mnt_model.py)."""
import random

import numpy as np
import pytest

import mnt_model as mm

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import (G1, G2, MNT4, MNT6, OUT_AFFINE, OUT_LIBFF, multi_exp_base_form_normal,  # noqa: E402
                       multi_exp_base_form_special, multi_exp_method_BDLO12, multi_exp_method_BDLO12_signed)

CURVES = [pytest.param(MNT4, G1, mm.MNT4, id="mnt4_g1"), pytest.param(MNT4, G2, mm.MNT4_G2, id="mnt4_g2"),
          pytest.param(MNT6, G1, mm.MNT6, id="mnt6_g1")]
UNSUPPORTED = -3


def _el(model, vals):
    return np.stack([model._coord_words(v) for v in vals])


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_field_ops(engine, curve, group, model):
    """coordinate-field ops (Fq, or Fq2 with non-residue 17) limb for limb in Montgomery form"""
    rng = random.Random(1)
    F, p = model.F, model.p
    rnd = lambda: F.of_comps([rng.randrange(p) for _ in range(model.deg)])
    a = [F.c(0), F.c(1), F.c(p - 1)] + [rnd() for _ in range(61)]
    b = [F.c(p - 1), F.c(0), F.c(p - 1)] + [rnd() for _ in range(61)]
    A, B = _el(model, a), _el(model, b)
    want = {0: [F.mul(x, y) for x, y in zip(a, b)], 1: [F.mul(x, x) for x in a], 2: [F.add(x, y) for x, y in zip(a, b)],
            3: [F.sub(x, y) for x, y in zip(a, b)], 4: [F.sub(F.zero(), x) for x in a]}
    for op, vals in want.items():
        got = engine.field_op(curve, group, op, A, B if op in (0, 2, 3) else None)
        assert (got == _el(model, vals)).all(), op
    got = engine.field_op(curve, group, 5, A[3:])
    assert (got == _el(model, [F.inv(x) for x in a[3:]])).all()


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_group_ops(engine, curve, group, model):
    P = model.random_points(6, seed=2)
    Q = model.random_points(6, seed=3)
    # P+Q, P+P, P+(-P), 0+P, P+0, 0+0
    lhs = P[:3] + [mm.INF, P[4], mm.INF]
    rhs = [Q[0], P[1], model.neg(P[2]), Q[3], mm.INF, mm.INF]
    zs = [1, 5, 7, 1, 3, 1]
    a = model.records(lhs, zs)
    for op, b in ((0, model.records(rhs, [2, 9, 4, 6, 1, 1])), (1, model.records(rhs))):
        for form in (OUT_LIBFF, OUT_AFFINE):
            got = engine.group_op(curve, group, op, a, b, out_form=form)
            assert [model.point(r) for r in got] == [model.add(x, y) for x, y in zip(lhs, rhs)], (op, form)
    got = engine.group_op(curve, group, 2, a, out_form=OUT_AFFINE)
    assert [model.point(r) for r in got] == [model.dbl(x) for x in lhs]


def _msm_case(model, n, seed):
    rng = random.Random(seed)
    pts = model.random_points(n, seed)
    ks = [rng.randrange(model.r) for _ in range(n)]
    return pts, ks


@pytest.mark.parametrize("curve,group,model", CURVES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 256, 257])
def test_multi_exp_forms(engine, curve, group, model, n):
    pts, ks = _msm_case(model, n, seed=n)
    want = model.msm(pts, ks)
    scal = model.scalars_mont(ks)
    zs = [random.Random(n + 100).randrange(1, model.p) for _ in range(n)]
    for form, bases in ((multi_exp_base_form_special, model.records(pts)),
                        (multi_exp_base_form_normal, model.records(pts, zs))):
        for method in (multi_exp_method_BDLO12, multi_exp_method_BDLO12_signed):
            for out_form in (OUT_LIBFF, OUT_AFFINE):
                got = engine.multi_exp(curve, group, bases, scal, method=method, base_form=form, out_form=out_form)
                assert model.point(got) == want, (form, method, out_form)


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_equal_and_opposite_bases(engine, curve, group, model):
    """Every base the same point, and the same point beside its negative: the buckets of k_accumulate meet P + P
    (the a != 0 doubling in the equal-point branch) and P + (-P)."""
    P = model.random_points(1, seed=5)[0]
    n = 4096
    rng = random.Random(6)
    ks = [rng.randrange(1, 64) for _ in range(n)]   # few distinct digits: long runs in one bucket
    want = model.mul(sum(ks), P)
    got = engine.multi_exp(curve, group, model.records([P] * n), model.scalars_mont(ks),
                           base_form=multi_exp_base_form_special)
    assert model.point(got) == want
    pts = [P if i % 2 == 0 else model.neg(P) for i in range(n)]
    want = model.mul(sum(k if i % 2 == 0 else -k for i, k in enumerate(ks)), P)
    got = engine.multi_exp(curve, group, model.records(pts), model.scalars_mont(ks), base_form=multi_exp_base_form_special)
    assert model.point(got) == want


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_window_sizes(engine, curve, group, model):
    pts, ks = _msm_case(model, 300, seed=7)
    ks[:3] = [0, 1, model.r - 1]
    want = model.msm(pts, ks)
    bases, scal = model.records(pts), model.scalars_mont(ks)
    for c in (2, 3, 5, 8, 13, 16, 20):
        got = engine.multi_exp(curve, group, bases, scal, base_form=multi_exp_base_form_special, window_bits=c)
        assert model.point(got) == want, c


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_filter_one_zero(engine, curve, group, model):
    pts, ks = _msm_case(model, 200, seed=8)
    for i in range(0, 200, 7):
        ks[i] = 0
    for i in range(3, 200, 11):
        ks[i] = 1
    got, stats = engine.multi_exp_filter_one_zero(curve, group, model.records(pts), model.scalars_mont(ks))
    assert model.point(got) == model.msm(pts, ks)
    assert stats["skipped"] == sum(k == 0 for k in ks) and stats["ones"] == sum(k == 1 for k in ks)


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_batch_exp_and_to_special(engine, curve, group, model):
    rng = random.Random(9)
    ks = [0, 1, model.r - 1] + [rng.randrange(model.r) for _ in range(61)]
    g = model.records([model.one])[0]
    for coeff in (None, 12345):
        cf = None if coeff is None else model.scalars_mont([coeff])[0]
        got = engine.batch_exp(curve, group, model.r.bit_length(), 5, g, model.scalars_mont(ks), coeff=cf)
        assert [model.point(r) for r in got] == [model.mul(k * (coeff or 1), model.one) for k in ks], coeff
    pts = model.random_points(8, seed=10) + [mm.INF]
    recs = model.records(pts, [3, 4, 5, 6, 7, 8, 9, 10, 1])
    sp = engine.batch_to_special(curve, group, recs)
    assert (sp == model.records(pts)).all()


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_batch_registered_and_contexts(engine, curve, group, model):
    cases = [_msm_case(model, 64, seed=20 + j) for j in range(3)]
    want = [model.msm(p, k) for p, k in cases]
    got = engine.multi_exp_batch(curve, group, [model.records(p) for p, _ in cases],
                                 [model.scalars_mont(k) for _, k in cases], base_form=multi_exp_base_form_special)
    assert [model.point(r) for r in got] == want
    pts, ks = cases[0]
    bases = model.records(pts)
    h = engine.register_bases(curve, group, bases, base_form=multi_exp_base_form_special)
    try:
        got = engine.multi_exp(curve, group, bases, model.scalars_mont(ks), base_form=multi_exp_base_form_special)
        assert model.point(got) == want[0]
    finally:
        engine.unregister_bases(h)
    e2 = libff_amd.Engine(0)
    got = libff_amd.multi_exp_multi([engine, e2], curve, group, bases, model.scalars_mont(ks),
                                    base_form=multi_exp_base_form_special)
    assert model.point(got) == want[0]


@pytest.mark.parametrize("curve,group,model,log_n", [
    pytest.param(*c.values, lg, id=f"{c.id}-2^{lg}") for c in CURVES for lg in (16, 20)] + [
    pytest.param(MNT4, G1, mm.MNT4, 22, id="mnt4_g1-2^22")])
def test_closed_form_gen_bases_seq(engine, curve, group, model, log_n):
    """sum_i k_i (i + 1) G over the device-generated bases (i + 1) G equals (sum_i k_i (i + 1) mod r) G."""
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    raw = rng.integers(0, 1 << 63, size=(n, mm.WORDS), dtype=np.uint64)
    raw[:, mm.WORDS - 1] &= np.uint64((1 << 40) - 1)   # below 2^296 < r: plain scalars
    bases = engine.gen_bases_seq(curve, group, n)
    assert model.point(bases[n - 1]) == model.mul(n, model.one)
    got = engine.multi_exp(curve, group, bases, raw, base_form=multi_exp_base_form_special, scalars_plain=True)
    total = 0
    for w in range(mm.WORDS):
        total += int(sum(int(v) * (i + 1) for i, v in enumerate(raw[:, w].tolist()))) << (64 * w)
    assert model.point(got) == model.mul(total, model.one)


@pytest.mark.parametrize("curve,group,model", CURVES)
def test_endomorphism_option_ignored(engine, curve, group, model):
    pts, ks = _msm_case(model, 300, seed=30)
    want = model.msm(pts, ks)
    for e in (-1, 0, 1, 2):
        assert libff_amd.plan(curve, group, 1 << 16, endomorphism=e)["endomorphism"] is False
        old = engine.endomorphism
        engine.endomorphism = e
        try:
            got = engine.multi_exp(curve, group, model.records(pts), model.scalars_mont(ks))
        finally:
            engine.endomorphism = old
        assert model.point(got) == want, e


def test_unsupported_paths(engine):
    import ctypes

    lib = libff_amd.load_library()
    out = (ctypes.c_size_t * 4)()
    assert lib.amdmsm_sizes(MNT6, G2, out) == UNSUPPORTED
    for group in (G1, G2):
        with pytest.raises(libff_amd.AmdMsmError):
            libff_amd.endomorphism_info(MNT4, group)
        with pytest.raises(libff_amd.AmdMsmError):
            engine.endomorphism_digits(MNT4, group, np.zeros((4, mm.WORDS), dtype=np.uint64), 8, 20)
    status = ctypes.c_uint(0)
    for curve, group in ((MNT4, G1), (MNT4, G2), (MNT6, G1)):
        rc = lib.amdmsm_disk_decode_device(engine.h, curve, group, None, ctypes.c_size_t(0), 1, None,
                                           ctypes.byref(status))
        assert rc == UNSUPPORTED
        rc = lib.amdmsm_multi_exp_stream_compressed_file(engine.h, curve, group, b"/nonexistent",
                                                         ctypes.c_size_t(0), None, ctypes.c_size_t(0),
                                                         ctypes.c_size_t(0), None, None)
        assert rc == UNSUPPORTED
