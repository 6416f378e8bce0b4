"""The digit pass of the bucket sort on a grid of its own choosing (group_vtable.h sort_digit_grid): every workgroup walks
several blocks of scalars, keeps one histogram in LDS and merges it into the global counters once.  On the device against
the CPU oracle with AMDMSM_SORT_DIGIT_WGS = 1 (one workgroup walks every block), 3 (5000 scalars are 5 blocks: two
workgroups with two blocks, the last block ragged) and unset (what the device holds at once).  The switch is read once per
process, so each setting is a child process of this very file (`python test_gpu_digit_grid.py --child ...`) under its own
time limit, one at a time; the child writes its results to a file and the parent compares them with the oracle's values,
computed once and shared by the three settings.  After a child that faulted, aborted or ran out of time every later test
of this file fails at once instead of starting more work on the device.

Cases, n in {1, 63, 1025, 5000} each:
  split  alt_bn128 G1, endomorphism = 0: the split, two digit columns per scalar (k_sort_digits mode 2)
  plain  bls12_377 G1, endomorphism = 0: no split on a curve group with a cofactor (mode 0)
  flat   alt_bn128 G1 through the precomputed table, c = 10: all digits of a scalar in one list (mode 1)
and
  sel    one batch of three MSMs over a shared scalar vector: 5000 bases with an index list with repeats, 1025 at an offset,
         63 with scalars of their own (k_sort_digits_sel)
  u8     5000 and 63 packed bytes (k_sort_digits_short<1>: 312 vectors of 16 and 8 single bytes are 320 work items, two
         blocks of 256), and 16000 bytes: 1000 items, at 3 workgroups four blocks of 256 -- the first workgroup walks two
         blocks shorter than a workgroup, the last block ragged
  fr     5000 and 63 Fr records below 2^40, promised (k_sort_digits_short<0>)
  equal  alt_bn128 G1, split, 5000 copies of one scalar: each window's histogram is one counter (two with the second half),
         its value the sum over every block of every workgroup
  big    the same with 18000 copies among 20001 scalars: more than big_thresh entries in one coarse bin, so k_sort_big_*
         take the counts the digit pass merged (5000 copies stay below that threshold of 16384)"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import libff_amd  # noqa: E402
from libff_amd import BatchItem  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIAL = libff_amd.multi_exp_base_form_special
NS = [1, 63, 1025, 5000]
FLAT_C = 10
SHARED_N = 1200
FR_BITS = 40
_fault = []
_want = {}


def _plain(curve, ints):
    fl = libff_amd.sizes(curve, 1)["fr_bytes"] // 8
    return np.array([[(int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(fl)] for v in ints], dtype=np.uint64)


def inputs(port):
    """name -> (kind, curve, bases, scalars, ...); seeded, the same in the parent and in every child"""
    rng = np.random.default_rng(20)
    cases = {}
    for n in NS:
        cases[f"split-{n}"] = ("msm", 0, port.bases_seq(0, 1, n, first=5), port.scalars_sha512(0, 100 + n, n))
        cases[f"plain-{n}"] = ("msm", 1, port.bases_seq(1, 1, n, first=5), port.scalars_sha512(1, 200 + n, n))
        cases[f"flat-{n}"] = ("flat", 0, port.bases_seq(0, 1, n, first=9), port.scalars_sha512(0, 300 + n, n))
    shared = port.scalars_sha512(0, 400, SHARED_N)
    idx = rng.integers(0, SHARED_N, 5000).astype(np.uint32)
    idx[:40] = idx[40]   # a run of repeats on top of the random ones
    cases["sel"] = ("sel", 0, [port.bases_seq(0, 1, 5000, first=2), port.bases_seq(0, 1, 1025, first=3), port.bases_seq(0, 1, 63, first=4)],
                    shared, idx, 17, port.scalars_sha512(0, 401, 63))
    cases["u8-16000"] = ("short", 0, port.bases_seq(0, 1, 16000, first=6), rng.integers(0, 256, 16000).astype(np.uint8))
    for n in (63, 5000):
        cases[f"u8-{n}"] = ("short", 0, port.bases_seq(0, 1, n, first=6), rng.integers(0, 256, n).astype(np.uint8))
        ints = [int(x) for x in rng.integers(0, 1 << FR_BITS, n, dtype=np.uint64)]
        ints[0] = (1 << FR_BITS) - 1
        cases[f"fr-{n}"] = ("short_fr", 0, port.bases_seq(0, 1, n, first=7), _plain(0, ints))
    one = port.scalars_sha512(0, 500, 1)
    cases["equal"] = ("msm", 0, port.bases_seq(0, 1, 5000, first=8), np.repeat(one, 5000, axis=0))
    big = port.scalars_sha512(0, 501, 20001)
    big[rng.permutation(20001)[:18000]] = one[0]
    cases["big"] = ("msm", 0, port.bases_seq(0, 1, 20001, first=8), big)
    return cases


def expected(port):
    """name -> list of oracle results; computed once"""
    if _want:
        return _want

    def msm(curve, bases, sc):
        return np.asarray(port.multi_exp(curve, 1, bases, sc, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True))

    for name, case in inputs(port).items():
        kind, curve = case[0], case[1]
        if kind in ("msm", "flat"):
            _want[name] = [msm(curve, case[2], case[3])]
        elif kind == "sel":
            bases, shared, idx, offset, own = case[2:]
            _want[name] = [msm(curve, bases[0], shared[idx.astype(np.int64)]), msm(curve, bases[1], shared[offset:offset + 1025]),
                           msm(curve, bases[2], own)]
        elif kind == "short":
            _want[name] = [msm(curve, case[2], port.fr_from_bigint(curve, _plain(curve, case[3])))]
        else:
            _want[name] = [msm(curve, case[2], port.fr_from_bigint(curve, case[3]))]
    return _want


def child_main(out_path, tmp_dir):
    from oracle import port

    port.build()
    port.lib()
    eng = libff_amd.Engine(0, endomorphism=0)
    got = {}
    for name, case in inputs(port).items():
        kind, curve = case[0], case[1]
        if kind == "msm":
            res = [eng.multi_exp(curve, 1, case[2], case[3], base_form=SPECIAL)]
        elif kind == "flat":
            tab = eng.precompute_table(curve, 1, case[2], FLAT_C)
            path = os.path.join(tmp_dir, f"{name}.bin")
            with open(path, "wb") as f:
                f.write(port.disk_write(curve, 1, tab).tobytes())
            res = [eng.multi_exp_stream_with_precompute_file(curve, 1, path, case[3], FLAT_C)]
            os.remove(path)
        elif kind == "sel":
            bases, shared, idx, offset, own = case[2:]
            items = [BatchItem(bases[0], index=idx), BatchItem(bases[1], offset=offset), BatchItem(bases[2], scalars=own)]
            res = eng.multi_exp_batch_items(curve, 1, items, shared, base_form=SPECIAL)
        elif kind == "short":
            res = [eng.multi_exp_short(curve, 1, case[2], case[3], base_form=SPECIAL)]
        else:
            res = [eng.multi_exp_short(curve, 1, case[2], case[3], bits=FR_BITS, base_form=SPECIAL, scalars_plain=True)]
        for j, r in enumerate(res):
            got[f"{name}/{j}"] = np.asarray(r)
        print(f"CASE {name}", flush=True)
    np.savez(out_path, **got)
    print("CHILD-DONE", flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _fault:
        pytest.fail(f"not started: an earlier child of this file faulted or timed out ({_fault[0]})")


def test_the_cases_are_what_they_claim():
    # 3 workgroups, 5000 scalars: 5 blocks, the last one ragged
    g = libff_amd.plan_sort_digit_grid(5000, 3)
    assert (g["block"], g["blocks"], g["grid"]) == (1024, 5, 3) and 5000 % 1024 != 0
    # 5000 bytes at a 16-byte boundary: 312 vectors of 16 and 8 single bytes, two blocks of 256 items
    g = libff_amd.plan_sort_digit_grid(312 + 8, 3, block_min=256)
    assert (g["block"], g["blocks"], g["grid"]) == (256, 2, 2)
    # 16000 bytes: 1000 vectors, four blocks of 256 on three workgroups, 232 items in the last
    g = libff_amd.plan_sort_digit_grid(1000, 3, block_min=256)
    assert (g["block"], g["blocks"], g["grid"]) == (256, 4, 3)
    assert libff_amd.plan(0, 1, 5000, endomorphism=0)["endomorphism"] and not libff_amd.plan(1, 1, 5000, endomorphism=0)["endomorphism"]
    geo = libff_amd.plan_sort(0, 1, 20001, endomorphism=0)
    assert 5000 < geo["big_thresh"] < 18000


@pytest.mark.parametrize("wgs", ["1", "3", None])
def test_digit_pass_grids(port, tmp_path, wgs):
    want = expected(port)
    out = tmp_path / "got.npz"
    env = dict(os.environ)
    env.pop("AMDMSM_SORT_DIGIT_WGS", None)
    if wgs is not None:
        env["AMDMSM_SORT_DIGIT_WGS"] = wgs
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(out), str(tmp_path)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _fault.append(f"wgs={wgs}: time limit")
        pytest.fail(f"child ran out of time; last output: {(e.stdout or b'')[-500:]!r}")
    if r.returncode != 0 or "CHILD-DONE" not in r.stdout:
        _fault.append(f"wgs={wgs}: exit status {r.returncode}")
        pytest.fail(f"child ended with status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    got = np.load(out)
    assert len(want) == 3 * len(NS) + 8
    bad = [f"{name}/{j}" for name, ws in want.items() for j, w in enumerate(ws) if not (got[f"{name}/{j}"] == w).all()]
    assert not bad, (wgs, bad)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2], sys.argv[3])
