#!/usr/bin/env python3
"""Generate tests/golden/mnt_disk.npz: the on-disk records the reference's own writer produces for MNT4-298 G1 / G2 and
MNT6-298 G1 -- group_write<encoding_binary, form_montgomery, compression_off> (curve_serialization.tcc:78-101), what
multi_exp_stream reads -- for seven elements per group, a zero among them.

Runs ONLY where the reference is mounted (LIBFF_REFERENCE, default /root/reference); the driver is compiled as
make_ffi_mnt_golden.py compiles its own.  The file holds data only.  Per group <g> in mnt4_g1, mnt4_g2, mnt6_g1:

  <g>/elems (7, 3 E) uint64   the elements as libff holds them: (X : Y : Z), Montgomery words, Z != 1 where the element
                              came out of an addition or a doubling
  <g>/disk_bytes (7 * 2 E * 8,) uint8   the records, one after the other
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_ffi_mnt_golden as base  # noqa: E402

DRIVER = r"""
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>
#include <libff/algebra/curves/mnt/mnt4/mnt4_pp.hpp>
#include <libff/algebra/curves/mnt/mnt6/mnt6_pp.hpp>
#include <libff/algebra/curves/curve_serialization.hpp>
#include <libff/common/profiling.hpp>

using namespace libff;

static void put(const char *g, const char *key, const void *p, size_t n)
{
    printf("%s/%s ", g, key);
    for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char *)p)[i]);
    printf("\n");
}

template<typename G, typename Fr> static void emit(const char *g)
{
    const G one = G::one();
    std::vector<G> v = {one, one.dbl(), Fr(17l) * one, G::zero(), -one, Fr(123456789l).inverse() * one, one + one.dbl()};
    for (const G &p : v) {
        std::string rec;
        rec.append((const char *)&p.X, sizeof(p.X));
        rec.append((const char *)&p.Y, sizeof(p.Y));
        rec.append((const char *)&p.Z, sizeof(p.Z));
        put(g, "elems", rec.data(), rec.size());
        std::ostringstream os(std::ios_base::out | std::ios_base::binary);
        group_write<encoding_binary, form_montgomery, compression_off>(p, os);
        const std::string s = os.str();
        put(g, "disk_bytes", s.data(), s.size());
    }
}

int main()
{
    inhibit_profiling_info = true;
    inhibit_profiling_counters = true;
    mnt4_pp::init_public_params();
    mnt6_pp::init_public_params();
    emit<mnt4_G1, mnt4_Fr>("mnt4_g1");
    emit<mnt4_G2, mnt4_Fr>("mnt4_g2");
    emit<mnt6_G1, mnt6_Fr>("mnt6_g1");
    return 0;
}
"""


def main():
    base.DRIVER = DRIVER
    rows = {}
    for line in base.run_driver().splitlines():
        if "/" not in line or " " not in line:
            continue
        key, hx = line.split(" ", 1)
        rows.setdefault(key, []).append(np.frombuffer(bytes.fromhex(hx.strip()), dtype=np.uint8))
    out = {}
    for key, vals in rows.items():
        if key.endswith("/elems"):
            out[key] = np.stack(vals).view("<u8").astype(np.uint64)
        else:
            out[key] = np.concatenate(vals)
    for g in ("mnt4_g1", "mnt4_g2", "mnt6_g1"):
        e, d = out[f"{g}/elems"], out[f"{g}/disk_bytes"]
        assert e.shape[0] == 7 and d.size == 7 * e.shape[1] // 3 * 2 * 8, g
        print(g, e.shape, d.shape)
    path = os.path.join(HERE, "mnt_disk.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
