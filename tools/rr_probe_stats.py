#!/usr/bin/env python3
"""What the reduced-radix probe tests (tests/test_gpu_rr_probe.py) feed the device, counted from the model alone (CPU):
per unit the operands of every op, the sides of every branch, the largest |j| of a same-x case and the per-field J.

    python tools/rr_probe_stats.py > profiles/rr_probe_operands.txt
"""
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import rr_model as rm   # noqa: E402


def main():
    for f in rm.FIELDS:
        s = rm.shape(f)
        reps = rm.zero_reps(f)
        print(f"{f}: B {s.B} L {s.L} D {s.D} filter K {s.K}; J {rm.zero_j_limit(s)}; representatives of zero and near misses "
              f"{dict(Counter(k for _, _, k in reps))}; first-point estimate {rm.first_sides(s, rm.first_words(f))}")
        for K in (64, s.K):
            print(f"    filter K = {K}: {rm.filter_sides(s, K, reps)}")
        for op in ("canon_product", "export_0", "export_d"):
            args = rm.limb_operands(f + "_g1", op)["args"]
            e = {"canon_product": None, "export_0": 32 * s.N, "export_d": 32 * s.N - s.D}[op]
            side = Counter(rm.canon_side(s, a[0][0] if e is None else rm.mul_pow2(s, a[0][0], e)) for a in args)
            print(f"    {op}: {dict(side)}")
    for name in rm.UNITS:
        u = rm.unit(name)
        s = u.s
        print(f"{name}:")
        print("    limb ops: " + ", ".join(f"{op} {len(rm.limb_operands(name, op)['args'])}" for op in rm.unit_ops(name)))
        madd = rm.madd_cases(name)
        print(f"    xyzz_madd_rr {len(madd)}: {dict(Counter((c['rung'], c['state']) for c in madd))}")
        js = [abs(j) for c in madd if c["rung"] in ("same", "opposite", "order_two") for j in rm.madd_same_x_multiple(name, c)]
        print(f"    largest |j| of a same-x case: {max(js)} (filter K {s.K})")
        print(f"    xyzz_rr_first 255, xyzz_rec_to_rho / export / export_rho {sum(1 for c in madd if not c['inf'])} each")
        print(f"    xyzz_add_rho {len(rm.add_cases(name))}: {dict(Counter(c['rung'] for c in rm.add_cases(name)))}")
        print(f"    xyzz_dbl_rho {len(rm.dbl_cases(name))}: {dict(Counter(c['rung'] for c in rm.dbl_cases(name)))}; "
              f"y = j p for j in {sorted(c['j'] for c in rm.dbl_cases(name) if c['j'] is not None)}")
        print(f"    jacobian {len(rm.jac_cases(name))}: {dict(Counter((c['op'], c['rung']) for c in rm.jac_cases(name)))}")


if __name__ == "__main__":
    main()
