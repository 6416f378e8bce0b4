"""Big-integer model of what the top window of an MSM plan can hold (shared by test_top_window_cpu.py and
test_gpu_top_window.py): the signed radix-2^c recoding of msm_group.hip for_each_signed_digit, the scalars that maximise
the halves of the endomorphism split, and the plan's own bound (amdmsm_plan_top_window)."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CURVE_NAMES = {0: "alt_bn128", 1: "bls12_377", 2: "bw6_761", 3: "bls12_381", 4: "mnt4", 5: "mnt6"}


def gen_params():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_params as gp_mod

    return gp_mod


def plan_top_window(curve, group, n, window_bits=0, endomorphism=0, scalars_plain=False):
    """amdmsm_plan_top_window as a dictionary: tb (bits of the top window's bucket index), shift (fine bits the sort drops
    there -- the value the sort launcher itself passes to its kernels), c, num_windows"""
    from libff_amd.engine import load_library

    lib = load_library()
    out = (ctypes.c_int * 4)()
    rc = lib.amdmsm_plan_top_window(int(curve), int(group), ctypes.c_size_t(n), int(window_bits), int(endomorphism),
                                    int(bool(scalars_plain)), out)
    assert rc == 0, f"amdmsm_plan_top_window: {rc}"
    return {"tb": out[0], "shift": out[1], "c": out[2], "num_windows": out[3]}


def signed_digits(m, c, W):
    """for_each_signed_digit on a non-negative integer, digit by digit"""
    mask, carry, out = (1 << c) - 1, 0, []
    for w in range(W):
        digit = ((m >> (c * w)) & mask) + carry
        overflow, cbit = (digit >> c) & 1, (digit >> (c - 1)) & 1
        out.append(0 if overflow else digit - (cbit << c))
        carry = overflow | cbit
    return out


def top_digit(m, c, W):
    """digit W - 1 of signed_digits(m, c, W) in one step: a window passes a carry on exactly when its digit plus the
    carry it received reaches 2^(c-1), i.e. when adding 2^(c-1) there carries out -- so the carry into the top window is
    the carry of m + (2^(c-1) in every lower window) out of those windows"""
    lowbits = c * (W - 1)
    bias = sum(1 << (c * w + c - 1) for w in range(W - 1))
    carry = ((m & ((1 << lowbits) - 1)) + bias) >> lowbits
    digit = ((m >> lowbits) & ((1 << c) - 1)) + carry
    if (digit >> c) & 1:
        return 0
    return digit - (((digit >> (c - 1)) & 1) << c)


def max_top_index_bits(values, c, W):
    """largest top_index_bits over many values (0 where none has an entry there), the window constants computed once"""
    lowbits = c * (W - 1)
    lowmask, cmask = (1 << lowbits) - 1, (1 << c) - 1
    bias = sum(1 << (c * w + c - 1) for w in range(W - 1))
    best = 0
    for m in values:
        digit = ((m >> lowbits) & cmask) + (((m & lowmask) + bias) >> lowbits)
        if (digit >> c) & 1 or digit == 0:
            continue
        d = digit - (((digit >> (c - 1)) & 1) << c)
        best = max(best, (abs(d) - 1).bit_length())
    return best


def top_index_bits(m, c, W):
    """bit length of the top window's bucket index |digit| - 1; None for a zero digit (no entry)"""
    d = top_digit(m, c, W)
    return None if d == 0 else (abs(d) - 1).bit_length()


def split_maximisers(cname):
    """(k with the largest |k1|, k with the largest |k2|) the split of this curve can produce, found from the lattice basis:
    the residue k - c1 v1 - c2 v2 is f1 v1 + f2 v2 with |f_i| <= 1/2 (+ the rounding error of the fixed-point
    constants), largest in the first / second coordinate at the corners where the two terms have the same sign there.
    Every integer point (u, v) of that parallelogram is the split of k = u + v lambda mod r."""
    gp_mod = gen_params()
    gp = gp_mod.glv_params(cname)
    r, lam = gp_mod.CURVES[cname]["r"], gp["lam"]
    (a1, b1), (a2, b2) = gp_mod.glv_lattice(r, lam)
    best = [None, None]
    for s1 in (1, -1):
        for s2 in (1, -1):
            # corners pulled inside by a factor 1 - 2^-e: the rounding of c1, c2 is exact only to about 2^-33
            for e in (24, 28, 30, 32, 34, 40, 64):
                u, v = ((s1 * a1 + s2 * a2) * ((1 << e) - 1)) >> (e + 1), ((s1 * b1 + s2 * b2) * ((1 << e) - 1)) >> (e + 1)
                k = (u + v * lam) % r
                k1, k2 = gp_mod.glv_split(gp, k)
                for j, h in enumerate((k1, k2)):
                    if best[j] is None or abs(h) > best[j][0]:
                        best[j] = (abs(h), k)
    return best[0][1], best[1][1]
