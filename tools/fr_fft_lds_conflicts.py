#!/usr/bin/env python3
"""LDS bank conflicts of k_fr_fft_pass (libff_amd/csrc/fr_ntt.hip) by the bank rule, for every pass shape, phase and stage.

The tile is 2^10 records, limb-pair major: pair w of record L is the 8-byte slot tile[w][sw(L)].  A wave's ds_read_b64 is
served in two groups of 32 lanes, the bank of a byte address a being (a / 4) % 64: a group is conflict-free when its 32
slots differ mod 32.  ds_write_b64 is served in four groups of 16 contiguous lanes with the bank (a / 4) % 32: a group is
conflict-free when its 16 slots differ mod 16.  Per access the script prints the worst number of lanes of a group that
share a bank (1 = conflict-free) with the swizzle and, for comparison, with the plain layout.

    python tools/fr_fft_lds_conflicts.py
    python tools/fr_fft_lds_conflicts.py --batch     k_fr_fft_pass_batch below 2^10 records: several whole vectors in a
                                                     tile, the vector index in the upper bits of the tile index
"""
import sys

LDS_LOG2, TPB = 10, 256


def sw(L):
    x = L >> 5
    return L ^ (x & 14) ^ ((x & 1) << 4) ^ ((x >> 4) * 17) ^ (((L >> 4) & 1) * 12)


def worst(records, swz, write):
    """records: for every lane-slot of the workgroup (thread order), the record index it touches"""
    lanes, mod = (16, 16) if write else (32, 32)
    w = 1
    for g in range(0, len(records), lanes):
        banks = {}
        for L in records[g:g + lanes]:
            banks.setdefault((swz(L) if swz else L) % mod, set()).add(L)
        w = max(w, max(len(v) for v in banks.values()))
    return w


def brev(x, t):
    return int(format(x, f"0{t}b")[::-1], 2) if t else 0


def pass_accesses(t, ls):
    """(name, record indices in thread order) of every LDS access of a full tile: t stages, stride 2^ls done before"""
    lc = LDS_LOG2 - t
    C, R, Et = 1 << lc, 1 << t, 1 << LDS_LOG2
    assert sorted(sw(L) for L in range(Et)) == list(range(Et))
    yield "load: put", list(range(Et))
    for j in range(t):
        lh = t - 1 - j
        h = 1 << lh
        lo = []
        for bf in range(Et // 2):
            cc, x = bf & (C - 1), bf >> lc
            i, blk = x & (h - 1), x >> lh
            lo.append((((blk << (lh + 1)) + i) << lc) | cc)
        for half, rec in (("lo", lo), ("hi", [L + (h << lc) for L in lo])):
            yield f"stage {j}: get {half}", rec
            yield f"stage {j}: put {half}", rec
    lsp = min(ls, lc)
    out = []
    for e in range(Et):
        ql, k2, pl = e & ((1 << lsp) - 1), (e >> lsp) & (R - 1), e >> (lsp + t)
        out.append((brev(k2, t) << lc) | ((pl << lsp) + ql))
    yield "store: get", out


def batch_accesses(log_n, t, ls):
    """the same for k_fr_fft_pass_batch below 2^10 records: the tile holds 2^(10 - log_n) whole vectors of 2^log_n records,
    the vector index in the upper bits of the tile index, and the pass does t of a vector's stages on 2^(log_n - t) columns"""
    le, lc = log_n, log_n - t
    C, R, Et = 1 << lc, 1 << t, 1 << LDS_LOG2
    yield "load: put", list(range(Et))
    for j in range(t):
        lh = t - 1 - j
        h = 1 << lh
        lo = []
        for bf in range(Et // 2):
            vl, bb = bf >> (le - 1), bf & ((1 << (le - 1)) - 1)
            cc, x = bb & (C - 1), bb >> lc
            i, blk = x & (h - 1), x >> lh
            lo.append((vl << le) | ((((blk << (lh + 1)) + i) << lc) | cc))
        for half, rec in (("lo", lo), ("hi", [L + (h << lc) for L in lo])):
            yield f"stage {j}: get {half}", rec
            yield f"stage {j}: put {half}", rec
    lsp = min(ls, lc)
    out = []
    for e in range(Et):
        vl, ee = e >> le, e & ((1 << le) - 1)
        ql, k2, pl = ee & ((1 << lsp) - 1), (ee >> lsp) & (R - 1), ee >> (lsp + t)
        out.append((vl << le) | (brev(k2, t) << lc) | ((pl << lsp) + ql))
    yield "store: get", out


def batch_shapes():
    """(log_n, t, ls) of every pass of a transform of fewer than 2^10 records, for every tile the plan allows"""
    seen = set()
    for log_n in range(1, LDS_LOG2):
        for tile in range(4, 9):
            passes = (log_n + tile - 1) // tile
            for k in range(passes):
                seen.add((log_n, tile if k < passes - 1 else log_n - (passes - 1) * tile, k * tile))
    return sorted(seen)


def main_batch():
    total = 0
    for log_n, t, ls in batch_shapes():
        rows = [(name, worst(rec, sw, "put" in name), worst(rec, None, "put" in name)) for name, rec in batch_accesses(log_n, t, ls)]
        bad = [(n, a, b) for n, a, b in rows if a > 1]
        total += len(bad)
        print(f"n = 2^{log_n} ({1 << (LDS_LOG2 - log_n)} vectors a tile), stages {t}, stride 2^{ls}: {len(rows)} accesses, "
              f"{len(bad)} with conflicts; without the swizzle {sum(1 for r in rows if r[2] > 1)} (worst {max(r[2] for r in rows)}-way)")
        for n, a, b in bad:
            print(f"    {n}: {a}-way (plain layout {b}-way)")
    print("accesses with conflicts:", total)


def main():
    if "--batch" in sys.argv[1:]:
        return main_batch()
    total = 0
    for t in range(4, 9):
        for ls in sorted({0, t, 2 * t}):
            rows = [(name, worst(rec, sw, "put" in name), worst(rec, None, "put" in name)) for name, rec in pass_accesses(t, ls)]
            bad = [(n, a, b) for n, a, b in rows if a > 1]
            total += len(bad)
            print(f"stages {t}, columns {1 << (LDS_LOG2 - t)}, stride 2^{ls}: {len(rows)} accesses, "
                  f"{len(bad)} with conflicts; without the swizzle {sum(1 for r in rows if r[2] > 1)} "
                  f"(worst {max(r[2] for r in rows)}-way)")
            for n, a, b in bad:
                print(f"    {n}: {a}-way (plain layout {b}-way)")
    print("accesses with conflicts:", total)


if __name__ == "__main__":
    main()
