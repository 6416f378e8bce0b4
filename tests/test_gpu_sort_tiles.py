"""The bucket sort's 16-bit staging (tile position + sign, bucket index) and the sizing of the fine pass's chunk, at the
shapes where they can go wrong: tile edges, a bin longer than the chunk, an oversized bin, digit signs, the flat mode of
the precomputed-table MSM and a wider group.  Every case is an MSM compared with the CPU oracle."""
import numpy as np
import pytest

import libff_amd

pytestmark = pytest.mark.gpu

SPECIAL = libff_amd.multi_exp_base_form_special
R_ALT_BN128 = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def engine_plain():
    """amdmsm_opts.endomorphism = -1: the scalars are never split"""
    return libff_amd.Engine(0, endomorphism=-1)


@pytest.fixture(scope="module")
def engine_split():
    """amdmsm_opts.endomorphism = 1: the split is permitted for every group that has one"""
    return libff_amd.Engine(0, endomorphism=1)


def mont_scalars(port, curve, ints):
    plain = np.zeros((len(ints), 4), dtype=np.uint64)
    for i, v in enumerate(ints):
        for j in range(4):
            plain[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return port.fr_from_bigint(curve, plain)


def check(eng, port, curve, group, bases, scalars, window_bits=0):
    want = port.multi_exp(curve, group, bases, scalars, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True)
    got = eng.multi_exp(curve, group, bases, scalars, libff_amd.multi_exp_method_BDLO12_signed, SPECIAL,
                        window_bits=window_bits)
    assert (got == want).all()


@pytest.mark.parametrize("n,split", [(8191, True), (8192, True), (8193, True), (16385, True), (16384, False)])
def test_tile_edges(engine, engine_plain, port, n, split):
    """c = 16: 2n = 16382, 16384, 16386, 32770 columns with the split (one entry short of a 16384-entry tile, one tile,
    one tile plus two, two tiles plus two) and n = 16384 columns without it."""
    geo = libff_amd.plan_sort(0, 1, n, window_bits=16, endomorphism=0 if split else -1)
    assert geo["columns"] == (2 * n if split else n)
    check(engine if split else engine_plain, port, 0, 1, port.bases_seq(0, 1, n, first=5), port.scalars_sha512(0, 40 + n, n),
          window_bits=16)


def test_bin_longer_than_the_chunk(engine_plain, port):
    """n = 2^16, no split, c = 10 (5 coarse bits: 2048 entries per bin expected): half of the scalars share their top 16
    bits, so one coarse bin of a window those bits cover holds 2^15 entries more -- longer than the fine pass's chunk,
    shorter than what is handed to the cooperative kernels."""
    n, c = 1 << 16, 10
    rng = np.random.default_rng(2024)
    top = 0x1234
    ints = [(top << 240) | int.from_bytes(rng.bytes(30), "little") for _ in range(n // 2)]
    ints += [int.from_bytes(rng.bytes(32), "little") % R_ALT_BN128 for _ in range(n // 2)]
    sc = mont_scalars(port, 0, ints)
    p = libff_amd.plan(0, 1, n, window_bits=c, endomorphism=-1)
    geo = libff_amd.plan_sort(0, 1, n, window_bits=c, endomorphism=-1)
    assert not p["endomorphism"] and p["c"] == c and geo["columns"] == n
    d = np.asarray(engine_plain.signed_digits(0, sc, c, p["num_windows"])).reshape(n, p["num_windows"]).astype(np.int64)
    # window 24 is bits 240 .. 249, the highest window that lies wholly inside the shared 16 bits (the short top window,
    # bits 250 .. 253 of a scalar below r, has a dozen buckets for any input: one coarse bin, sorted cooperatively)
    w = 24
    assert w * c >= 240 and (w + 1) * c <= 256 and w < p["num_windows"]
    col = d[:, w]
    idx = np.abs(col[col != 0]) - 1
    longest = int(np.bincount(idx >> geo["fine_bits"], minlength=1 << geo["coarse_bits"]).max())
    assert longest >= n // 2
    assert geo["chunk_cap"] < longest <= geo["big_thresh"], (geo, longest)
    check(engine_plain, port, 0, 1, port.bases_seq(0, 1, n, first=1), sc, window_bits=c)


def test_oversized_bin(engine, port):
    """n = 2^15 equal scalars: every window is one bucket, sorted by k_sort_big_* through the shared staging layout"""
    n = 1 << 15
    geo = libff_amd.plan_sort(0, 1, n)
    assert geo["columns"] > geo["big_thresh"]
    sc = np.repeat(port.scalars_sha512(0, 77, 1), n, axis=0)
    check(engine, port, 0, 1, port.bases_seq(0, 1, n, first=9), sc)


def test_digit_signs(engine_plain, port):
    """c = 16 without the split: every digit of an even window is negative (its 16 bits are >= 2^15), every digit of an odd
    window positive (< 2^15 - 1, plus the carry) -- the sign travels through the staging in bit 15 of the position.
    20000 scalars: a full tile and a part of a second one."""
    n, c = 20000, 16
    rng = np.random.default_rng(7)
    ints = []
    for _ in range(n):
        v = 0
        for w in range(16):
            chunk = int(rng.integers(0x8000, 0x10000)) if w % 2 == 0 else int(rng.integers(0, 0x2FFF if w == 15 else 0x7FFF))
            v |= chunk << (16 * w)
        ints.append(v)
    assert max(ints) < R_ALT_BN128
    sc = mont_scalars(port, 0, ints)
    p = libff_amd.plan(0, 1, n, window_bits=c, endomorphism=-1)
    d = np.asarray(engine_plain.signed_digits(0, sc, c, p["num_windows"])).reshape(n, p["num_windows"]).astype(np.int64)
    assert (d[:, 0:16:2] < 0).all() and (d[:, 1:16:2] > 0).all()
    check(engine_plain, port, 0, 1, port.bases_seq(0, 1, n, first=2), sc, window_bits=c)


def test_flat_mode_precomputed(engine, port):
    """msm_precomputed_device, n = 2^12, c = 16: one list of n * D entries whose payloads i * D + j are rebuilt from the
    tile position."""
    curve, group, n, c = 0, 1, 1 << 12, 16
    D = libff_amd.precompute_num_digits(curve, c)
    bases = port.bases_seq(curve, group, n, first=13)
    sc = port.scalars_sha512(curve, 4242, n)
    tab = engine.precompute_table(curve, group, bases, c, num_digits=D)
    want = port.multi_exp_precompute(curve, group, tab, sc, c)
    z = libff_amd.sizes(curve, group)
    d_src, d_tab = engine.malloc(tab.nbytes), engine.malloc(tab.shape[0] * z["affine_bytes"])
    d_sc, d_out = engine.malloc(sc.nbytes), engine.malloc(z["g_bytes"])
    try:
        engine.h2d(d_src, tab)
        engine.h2d(d_sc, sc)
        engine.import_bases_device(curve, group, d_src, tab.strides[0], SPECIAL, tab.shape[0], d_tab)
        engine.msm_precomputed_device(curve, group, d_tab, d_sc, n, c, D, d_out, out_form=libff_amd.OUT_AFFINE)
        engine.synchronize()
        out = np.zeros(z["g_bytes"] // 8, dtype=np.uint64)
        engine.d2h(out, d_out)
    finally:
        for p in (d_src, d_tab, d_sc, d_out):
            engine.free(p)
    assert (out == want).all()


def test_wider_group_bls12_377_g2(engine_split, port):
    """bls12_377 G2, n = 8193, the split permitted: 16386 columns"""
    n = 8193
    assert libff_amd.plan(1, 2, n, endomorphism=1)["endomorphism"]
    check(engine_split, port, 1, 2, port.bases_seq(1, 2, n, first=3), port.scalars_sha512(1, 99, n))
