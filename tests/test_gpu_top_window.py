"""The top window sorted by its real width (group_vtable.h sort_top_shift), on the device against the CPU oracle, with the
shift in force and with AMDMSM_SORT_TOPSHIFT=0.  The switch is read once per process, so each run is a child process of
this very file (`python test_gpu_top_window.py --child ...`) under its own time limit, one at a time; the child writes its
result to a file and the parent compares it with port.multi_exp, computed once per case.  After a child that faulted,
aborted or ran out of time every later test of this file fails at once instead of starting more work on the device.

Scalars of every case: seeded random ones, r - 1, 1, 0, the scalars that maximise |k1| and |k2| of the split 300 times each
(the top window's last used bin and last used bucket), and many copies of one scalar (one bin far longer than the fine
pass's chunk with the shift in force): 5000 of the 12293, 1500 of the 4099 of the wider group.

  a  alt_bn128 G1, split, c = 16: 8 windows, the top one holds 13.8 of 15 index bits -- one fine bit dropped
  b  alt_bn128 G1, split, c = 13: 10 windows, the top one holds 125.8 - 9 * 13 = 8.8 of 12 -- three
  c  alt_bn128 G1, no split, c = 16: 16 windows, 14 of 15 -- one
  d  bls12_377 G2, split permitted, the planner's own window size
  e  alt_bn128 G1, no split, c = 13, PLAIN scalars that are not reduced: 20 windows cover 260 bits, so every integer of
     256 bits is exact input (k means k mod r); a quarter of the scalars have bit 255 set, 2^256 - 1 among them.  The bound
     is then the word length: 256 - 19 * 13 = 9 of 12 bits, three dropped, and bit 255 reaches the top bucket of that range
  f  alt_bn128 G1, split, c = 16, n = 20001 with 18000 copies of one scalar: more than big_thresh entries in one bin of
     every window, the top one included -- k_sort_big_hist / _scan / _scatter with the shift
  g  alt_bn128 G1, split, c = 20: 7 windows, the top one holds 6 of 19 bits and the shift takes ALL nine fine bits
     (one fine bucket per bin), the shape of the 2^26 plan"""
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
import top_window as tw  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIAL = libff_amd.multi_exp_base_form_special
# name: (curve, group, n, endomorphism, window_bits, copies of one scalar)
CASES = {
    "a": (0, 1, 12293, 0, 16, 5000),
    "b": (0, 1, 12293, 0, 13, 5000),
    "c": (0, 1, 12293, -1, 16, 5000),
    "d": (1, 2, 4099, 1, 0, 1500),
    "e": (0, 1, 12293, -1, 13, 5000),
    "f": (0, 1, 20001, 0, 16, 18000),
    "g": (0, 1, 12293, 0, 20, 5000),
}
PLAIN = ("e",)   # scalars passed as plain integers (amdmsm_opts.scalars_plain), not reduced mod r
_fault = []
_want = {}


def case_scalars(name):
    """plain integers of the case, in a seeded shuffled order"""
    curve, group, n, endo, c, copies = CASES[name]
    gp_mod = tw.gen_params()
    cname = tw.CURVE_NAMES[curve]
    r = gp_mod.CURVES[cname]["r"]
    k1max, k2max = tw.split_maximisers(cname)
    rng = np.random.default_rng(600 + ord(name))
    one = int.from_bytes(rng.bytes(48), "little") % r
    ks = [r - 1, 1, 0] + [k1max] * 300 + [k2max] * 300 + [one] * copies
    ks += [int.from_bytes(rng.bytes(48), "little") % r for _ in range(n - len(ks))]
    assert len(ks) == n
    if name in PLAIN:
        bits = libff_amd.sizes(curve, 1)["fr_bytes"] * 8
        top = 1 << (bits - 1)
        ks = [(k | top) if i % 4 == 0 else k for i, k in enumerate(ks)]
        ks[0], ks[1], ks[2] = (1 << bits) - 1, top, r
    return [ks[i] for i in rng.permutation(n)]


def words(curve, ints):
    fl = libff_amd.sizes(curve, 1)["fr_bytes"] // 8
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(fl)] for v in ints], dtype=np.uint64)


def case_inputs(port, name, reduced=False):
    """bases and the scalars the device gets: Montgomery residues, or for a PLAIN case the integers as they are;
    reduced: what the oracle gets, always the Montgomery residues of k mod r"""
    curve, group, n, endo, c, copies = CASES[name]
    ks = case_scalars(name)
    bases = port.bases_seq(curve, group, n, first=7)
    if name in PLAIN and not reduced:
        return bases, words(curve, ks)
    r = tw.gen_params().CURVES[tw.CURVE_NAMES[curve]]["r"]
    return bases, port.fr_from_bigint(curve, words(curve, [k % r for k in ks]))


def child_main(name, out_path):
    from oracle import port

    port.build()
    port.lib()
    curve, group, n, endo, c, copies = CASES[name]
    bases, sc = case_inputs(port, name)
    t = tw.plan_top_window(curve, group, n, window_bits=c, endomorphism=endo, scalars_plain=name in PLAIN)
    print(f"SHIFT {t['shift']} TB {t['tb']} C {t['c']} W {t['num_windows']}", flush=True)
    eng = libff_amd.Engine(0, endomorphism=endo)
    got = eng.multi_exp(curve, group, bases, sc, libff_amd.multi_exp_method_BDLO12_signed, SPECIAL, window_bits=c,
                        scalars_plain=name in PLAIN)
    np.save(out_path, np.asarray(got))
    print("CHILD-DONE", flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _fault:
        pytest.fail(f"not started: an earlier child of this file faulted or timed out ({_fault[0]})")


def expected(port, name):
    if name not in _want:
        curve, group, n, endo, c, copies = CASES[name]
        bases, sc = case_inputs(port, name, reduced=True)
        _want[name] = port.multi_exp(curve, group, bases, sc, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True)
    return _want[name]


@pytest.mark.parametrize("topshift", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_top_window_cases(port, tmp_path, name, topshift):
    curve, group, n, endo, c, copies = CASES[name]
    p = libff_amd.plan(curve, group, n, window_bits=c, endomorphism=endo)
    assert p["endomorphism"] == (name not in "ce")
    t = tw.plan_top_window(curve, group, n, window_bits=c, endomorphism=endo, scalars_plain=name in PLAIN)
    geo = libff_amd.plan_sort(curve, group, n, window_bits=c, endomorphism=endo)
    assert t["shift"] == min(geo["fine_bits"], t["c"] - 1 - t["tb"]) >= 1
    if name != "d":
        assert (p["num_windows"], t["tb"], t["shift"]) == {"a": (8, 14, 1), "b": (10, 9, 3), "c": (16, 14, 1), "e": (20, 9, 3),
                                                           "f": (8, 14, 1), "g": (7, 6, 9)}[name]
    if name == "e":
        # unreduced plain scalars: the windows cover the whole word, bit 255 lands in the top window's highest used bucket
        assert t["c"] * t["num_windows"] > 256
        assert max(tw.top_index_bits(k, t["c"], t["num_windows"]) or 0 for k in case_scalars(name)) == t["tb"]
    if name == "f":
        assert copies > geo["big_thresh"]
    if name == "g":
        assert t["shift"] == geo["fine_bits"]
    # the maximisers reach the top window's last used bucket: an index of tb or tb - 1 bits
    if p["endomorphism"]:
        gp_mod = tw.gen_params()
        gp = gp_mod.glv_params(tw.CURVE_NAMES[curve])
        halves = [abs(h) for k in tw.split_maximisers(tw.CURVE_NAMES[curve]) for h in gp_mod.glv_split(gp, k)]
        assert t["tb"] - 1 <= max(tw.top_index_bits(m, t["c"], t["num_windows"]) or 0 for m in halves) <= t["tb"]
    want = expected(port, name)
    out = tmp_path / "got.npy"
    env = dict(os.environ, AMDMSM_SORT_TOPSHIFT=str(topshift))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, str(out)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _fault.append(f"{name} topshift={topshift}: time limit")
        pytest.fail(f"child ran out of time; last output: {(e.stdout or b'')[-500:]!r}")
    if r.returncode != 0 or "CHILD-DONE" not in r.stdout:
        _fault.append(f"{name} topshift={topshift}: exit status {r.returncode}")
        pytest.fail(f"child ended with status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    assert f"SHIFT {t['shift'] if topshift else 0} TB {t['tb']} " in r.stdout, r.stdout
    assert (np.load(out) == want).all()


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_split_digits_of_the_maximisers(engine, curve):
    """the split's carry chains on the scalars with the longest halves (and their neighbours): digits of both halves from
    the device against the big-integer split and recoding"""
    gp_mod = tw.gen_params()
    cname = tw.CURVE_NAMES[curve]
    gp, r = gp_mod.glv_params(cname), gp_mod.CURVES[cname]["r"]
    ks = [(k + d) % r for k in tw.split_maximisers(cname) for d in (-1, 0, 1)] + [r - 1, (r - 1) // 2, 0, 1]
    fl = libff_amd.sizes(curve, 1)["fr_bytes"] // 8
    plain = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(fl)] for v in ks], dtype=np.uint64)
    for c in (13, 16):
        W = libff_amd.plan(curve, 1, len(ks), window_bits=c, endomorphism=2)["num_windows"]
        d = engine.endomorphism_digits(curve, 1, plain, c, W, scalars_plain=True)
        for i, k in enumerate(ks):
            for half, h in enumerate(gp_mod.glv_split(gp, k)):
                want = [(-x if h < 0 else x) for x in tw.signed_digits(abs(h), c, W)]
                assert [int(x) for x in d[i, half]] == want, (cname, c, i, half)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2], sys.argv[3])
