#!/usr/bin/env python3
"""Generate tests/golden/plan_layout.json: what amdmsm_plan_ex and amdmsm_plan_short answer over a grid of requests.

    python tests/golden/make_plan_layout.py <libamdmsm.so> [out.json]

The fixture pins the MSM plan -- window size, window count, buckets, the workspace's size and the split decision --
across changes that must not move it, so <libamdmsm.so> is a library built at the commit BEFORE such a change.  Without
[out.json] the table goes to standard output, which is how tests/test_plan_layout_cpu.py asks the library under test.

The plan depends on the lanes the device holds at once, so the table is taken with no device visible
(HIP_VISIBLE_DEVICES="" and ROCR_VISIBLE_DEVICES="", set by the caller before this process starts): the query then takes
its fixed fallback, 256 CUs x 4 workgroups, on any machine.

Per group "<curve>,<group>" one row per request, in the order of `requests()`: [rc, c, W, buckets, workspace_bytes,
endomorphism_used], the five values 0 where rc != 0 (a refusal is compared as its return code).
"""
import ctypes
import json
import os
import sys

GROUPS = [(0, 1), (1, 2), (2, 1), (4, 1)]   # alt_bn128 G1, bls12_377 G2, bw6_761 G1, mnt4 G1
SIZES = [1, 63, 64, 65, 1000, 1 << 16, 3 << 18, 1 << 20, 1 << 23]
WINDOW_BITS = [0, 2, 9, 10, 16, 22, 24]
ENDOMORPHISM = [-1, 1, 2, 0]                # off, on (permitted / at every size), auto
SHORT_BITS = [0, 1, 32, 64]                 # 0: amdmsm_plan_ex, else amdmsm_plan_short with that many bits


def requests():
    return [(n, wb, endo, bits) for n in SIZES for wb in WINDOW_BITS for endo in ENDOMORPHISM for bits in SHORT_BITS]


def collect(so_path):
    assert os.environ.get("HIP_VISIBLE_DEVICES") == "" and os.environ.get("ROCR_VISIBLE_DEVICES") == "", \
        "the table is taken with no device visible"
    lib = ctypes.CDLL(so_path)
    plans = {}
    for curve, group in GROUPS:
        rows = []
        for n, wb, endo, bits in requests():
            c, w, used, b, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_size_t(0)
            out = (ctypes.byref(c), ctypes.byref(w), ctypes.byref(b), ctypes.byref(ws), ctypes.byref(used))
            if bits:
                rc = lib.amdmsm_plan_short(curve, group, ctypes.c_size_t(n), wb, endo, bits, *out)
            else:
                rc = lib.amdmsm_plan_ex(curve, group, ctypes.c_size_t(n), wb, endo, *out)
            rows.append([rc, c.value, w.value, b.value, ws.value, used.value] if rc == 0 else [rc, 0, 0, 0, 0, 0])
        plans[f"{curve},{group}"] = rows
    return {"sizes": SIZES, "window_bits": WINDOW_BITS, "endomorphism": ENDOMORPHISM, "short_bits": SHORT_BITS,
            "plans": plans}


if __name__ == "__main__":
    table = collect(sys.argv[1])
    text = json.dumps(table, separators=(",", ":")).replace("],[", "],\n[")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
