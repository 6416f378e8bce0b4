// Self-test of the loose-limb Horner chain (libff_amd/csrc/wide28.cuh: to28, jac_dbl_28, jac_add_28, from28) against
// the canonical lane-split chain (wide.cuh: jac_dbl_wide, jac_add_wide), word for word after from28, for the three
// fields of the lazy chain; then the time of one addition / doubling / conversion pair in either form.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Ilibff_amd/csrc tools/lazy_chain_test.hip -o /tmp/lazy_chain_test && /tmp/lazy_chain_test
// A test is a start point A, an operand B and up to 32 operations: 1 double, 2 add B, 3 add A, 4 add -A, 5 add infinity.
// Single additions cover random points, P + P, P + (-P), P + 0, 0 + P, 0 + 0 with coordinates at the edges (p - 1, p - 2,
// all-ones words, single bits, zero X or Y); chains mix up to 22 doublings and 8 additions in random order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "curve_params.h"
#include "ec.cuh"
#include "wide.cuh"
#include "wide28.cuh"

using namespace amdmsm;

constexpr int OPS = 32;

template <class P>
__global__ void __launch_bounds__(64) k_chain(const uint32_t* in, const unsigned char* ops, uint32_t* out_lazy, uint32_t* out_ref,
                                              int tests) {
    constexpr int N = P::N;
    const WideEnv<P> e = wide_env<P>();
    const Env28<P, 10> v = env28<P, 10>(e);
    const uint32_t sub4 = tab28_sel(A28<P>::SUB4, e.j);
    const uint32_t row = (threadIdx.x & 63u) >> 4;
    for (int t = 0; t < tests; ++t) {
        const uint32_t* a = in + (size_t)t * 6 * N;
        const uint32_t* b = a + 3 * N;
        const uint32_t ax = e.valid ? a[e.j] : 0u, ay = e.valid ? a[N + e.j] : 0u, az = e.valid ? a[2 * N + e.j] : 0u;
        const uint32_t bx = e.valid ? b[e.j] : 0u, by = e.valid ? b[N + e.j] : 0u, bz = e.valid ? b[2 * N + e.j] : 0u;
        const uint32_t nay = wide_sub<P>(e, 0u, ay);
        // canonical chain
        uint32_t X = ax, Y = ay, Z = az;
        // lazy chain: row r converts coordinate r
        auto conv = [&](uint32_t x, uint32_t y, uint32_t z, uint32_t& X28, uint32_t& Y28, uint32_t& Z28) {
            const uint32_t r = to28(v, row == 0 ? x : (row == 1 ? y : (row == 2 ? z : 0u)));
            X28 = from_row(r, 0);
            Y28 = from_row(r, 1);
            Z28 = from_row(r, 2);
        };
        uint32_t X28, Y28, Z28, BX, BY, BZ, AX, AY, AZ, NY, d0, d1;
        conv(ax, ay, az, X28, Y28, Z28);
        AX = X28, AY = Y28, AZ = Z28;
        conv(bx, by, bz, BX, BY, BZ);
        conv(ax, nay, az, d0, NY, d1);
        for (int k = 0; k < OPS; ++k) {
            const int op = ops[(size_t)t * OPS + k];   // wave-uniform
            if (op == 0) break;
            if (op == 1) {
                jac_dbl_wide<P>(e, X, Y, Z);
                jac_dbl_28<P>(v, X28, Y28, Z28);
            } else if (op == 2) {
                jac_add_wide<P>(e, X, Y, Z, bx, by, bz);
                jac_add_28<P>(v, sub4, X28, Y28, Z28, BX, BY, BZ);
            } else if (op == 3) {
                jac_add_wide<P>(e, X, Y, Z, ax, ay, az);
                jac_add_28<P>(v, sub4, X28, Y28, Z28, AX, AY, AZ);
            } else if (op == 4) {
                jac_add_wide<P>(e, X, Y, Z, ax, nay, az);
                jac_add_28<P>(v, sub4, X28, Y28, Z28, AX, NY, AZ);
            } else {
                jac_add_wide<P>(e, X, Y, Z, ax, ay, 0u);
                jac_add_28<P>(v, sub4, X28, Y28, Z28, AX, AY, 0u);
            }
        }
        const uint32_t r = from28(v, row == 0 ? X28 : (row == 1 ? Y28 : Z28));
        const uint32_t LX = from_row(r, 0), LY = from_row(r, 1), LZ = from_row(r, 2);
        if (threadIdx.x < (unsigned)N) {
            uint32_t* o = out_lazy + (size_t)t * 3 * N;
            uint32_t* q = out_ref + (size_t)t * 3 * N;
            o[e.j] = LX;
            o[N + e.j] = LY;
            o[2 * N + e.j] = LZ;
            q[e.j] = X;
            q[N + e.j] = Y;
            q[2 * N + e.j] = Z;
        }
    }
}

// mode 0: jac_add_wide, 1: jac_add_28, 2: jac_dbl_wide, 3: jac_dbl_28, 4: to28 + from28 of the three coordinates
template <class P>
__global__ void __launch_bounds__(64) k_time(const uint32_t* in, uint32_t* out, int mode, int iters) {
    constexpr int N = P::N;
    const WideEnv<P> e = wide_env<P>();
    const Env28<P, 10> v = env28<P, 10>(e);
    const uint32_t sub4 = tab28_sel(A28<P>::SUB4, e.j);
    const uint32_t row = (threadIdx.x & 63u) >> 4;
    uint32_t X = e.valid ? in[e.j] : 0u, Y = e.valid ? in[N + e.j] : 0u, Z = e.valid ? in[2 * N + e.j] : 0u;
    const uint32_t bx = e.valid ? in[3 * N + e.j] : 0u, by = e.valid ? in[4 * N + e.j] : 0u, bz = e.valid ? in[5 * N + e.j] : 0u;
    if (mode == 0) {
        for (int i = 0; i < iters; ++i) jac_add_wide<P>(e, X, Y, Z, bx, by, bz);
    } else if (mode == 2) {
        for (int i = 0; i < iters; ++i) jac_dbl_wide<P>(e, X, Y, Z);
    } else if (mode == 4) {
        for (int i = 0; i < iters; ++i) {
            uint32_t r = to28(v, row == 0 ? X : (row == 1 ? Y : Z));
            r = from28(v, r);
            X = from_row(r, 0);
            Y = from_row(r, 1);
            Z = from_row(r, 2);
        }
    } else {
        uint32_t r = to28(v, row == 0 ? X : (row == 1 ? Y : Z));
        uint32_t X28 = from_row(r, 0), Y28 = from_row(r, 1), Z28 = from_row(r, 2);
        r = to28(v, row == 0 ? bx : (row == 1 ? by : bz));
        const uint32_t BX = from_row(r, 0), BY = from_row(r, 1), BZ = from_row(r, 2);
        if (mode == 1) for (int i = 0; i < iters; ++i) jac_add_28<P>(v, sub4, X28, Y28, Z28, BX, BY, BZ);
        else for (int i = 0; i < iters; ++i) jac_dbl_28<P>(v, X28, Y28, Z28);
        r = from28(v, row == 0 ? X28 : (row == 1 ? Y28 : Z28));
        X = from_row(r, 0);
        Y = from_row(r, 1);
        Z = from_row(r, 2);
    }
    if (threadIdx.x < (unsigned)N) {
        out[e.j] = X;
        out[N + e.j] = Y;
        out[2 * N + e.j] = Z;
    }
}

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t err_ = (x);                                                    \
        if (err_ != hipSuccess) {                                                 \
            printf("%s: %s\n", #x, hipGetErrorString(err_));                      \
            return 1000000;                                                       \
        }                                                                         \
    } while (0)

template <class P>
int run(const char* name) {
    constexpr int N = P::N;
    const int tests = 3000;
    std::vector<uint32_t> in((size_t)tests * 6 * N);
    std::vector<unsigned char> ops((size_t)tests * OPS, 0);
    uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)N * 0x2545f4914f6cdd1dull;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 16);
    };
    auto element = [&](uint32_t* w, int kind) {
        for (int i = 0; i < N; ++i) {
            uint32_t x = rnd();
            if (kind == 0) x = 0xffffffffu;           // all-ones words (reduced below at the top)
            if (kind == 1) x = 0;                      // zero coordinate
            if (kind == 2 || kind == 3) x = P::P[i];   // p - 1, p - 2
            if (kind == 4) x = 0;                      // a single bit
            w[i] = x;
        }
        if (kind == 2 || kind == 3) {                  // with the borrow: bls12_377's p ends in ...00000001
            uint32_t take = kind == 2 ? 1u : 2u;
            for (int i = 0; i < N && take; ++i) {
                const uint32_t before = w[i];
                w[i] -= take;
                take = before < take ? 1u : 0u;
            }
        }
        if (kind == 4) {
            const uint32_t bit = rnd() % (uint32_t)(P::BITS - 1);
            w[bit / 32] = 1u << (bit % 32);
        }
        if (kind != 2 && kind != 3 && kind != 4) w[N - 1] %= P::P[N - 1];
    };
    for (int t = 0; t < tests; ++t) {
        uint32_t* a = &in[(size_t)t * 6 * N];
        for (int c = 0; c < 6; ++c) {
            int kind = (int)(rnd() % 10);              // 5..9: random
            if ((c == 2 || c == 5) && kind == 1) kind = 9;   // Z = 0 comes from the operations below
            element(a + c * N, kind);
        }
        unsigned char* o = &ops[(size_t)t * OPS];
        const int shape = t % 12;
        if (shape < 6) {
            // single additions: B, P + P, P + (-P), P + 0, 0 + P, 0 + 0
            if (shape == 4 || shape == 5) for (int i = 0; i < N; ++i) a[2 * N + i] = 0;
            o[0] = shape == 0 ? 2 : (shape == 1 ? 3 : (shape == 2 ? 4 : (shape == 3 ? 5 : (shape == 4 ? 2 : 5))));
            if (t % 24 >= 12) o[1] = 1;                // and a doubling of the result
        } else {
            // chains: up to 22 doublings and 8 additions in random order
            int nd = (int)(rnd() % 23), na = 1 + (int)(rnd() % 8), k = 0;
            while (nd + na > 0 && k < OPS - 1) {
                const bool add = na > 0 && (nd == 0 || rnd() % (uint32_t)(nd + na) < (uint32_t)na);
                if (add) {
                    const uint32_t w = rnd() % 8;
                    o[k++] = w < 4 ? 2 : (w == 4 ? 3 : (w == 5 ? 4 : (w == 6 ? 5 : 3)));
                    --na;
                } else {
                    o[k++] = 1;
                    --nd;
                }
            }
        }
    }
    uint32_t *d_in, *d_l, *d_r;
    unsigned char* d_ops;
    const size_t ob = (size_t)tests * 3 * N * 4;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_ops, ops.size()));
    CHECK(hipMalloc(&d_l, ob));
    CHECK(hipMalloc(&d_r, ob));
    CHECK(hipMemset(d_l, 0, ob));
    CHECK(hipMemset(d_r, 0xff, ob));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_ops, ops.data(), ops.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_chain<P>, dim3(1), dim3(64), 0, 0, d_in, d_ops, d_l, d_r, tests);
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> l(ob / 4), r(ob / 4);
    CHECK(hipMemcpy(l.data(), d_l, ob, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(r.data(), d_r, ob, hipMemcpyDeviceToHost));
    int bad = 0, infs = 0;
    for (int t = 0; t < tests; ++t) {
        const size_t o = (size_t)t * 3 * N;
        bool zinf = true;
        for (int i = 0; i < N; ++i) zinf = zinf && r[o + 2 * N + i] == 0;
        infs += zinf;
        bool same = true;
        for (int i = 0; i < 3 * N; ++i) same = same && l[o + i] == r[o + i];
        if (!same && bad++ == 0) {
            printf("%s first mismatch test %d (shape %d)\n  lazy:", name, t, t % 12);
            for (int i = 3 * N - 1; i >= 0; --i) printf(" %08x", l[o + i]);
            printf("\n  ref: ");
            for (int i = 3 * N - 1; i >= 0; --i) printf(" %08x", r[o + i]);
            printf("\n");
        }
    }
    printf("%s: %d chains (%d end at infinity), loose limbs vs canonical, X Y Z word for word: %s (%d differ)\n", name, tests, infs,
           bad ? "FAIL" : "ok", bad);
    // timings: one wave, dependent chain
    const int iters = 2000;
    const char* what[5] = {"jac_add_wide", "jac_add_28", "jac_dbl_wide", "jac_dbl_28", "to28 + from28"};
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int mode = 0; mode < 5; ++mode) {
        hipLaunchKernelGGL(k_time<P>, dim3(1), dim3(64), 0, 0, d_in + 6 * N * 6, d_l, mode, 10);
        CHECK(hipDeviceSynchronize());
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_time<P>, dim3(1), dim3(64), 0, 0, d_in + 6 * N * 6, d_l, mode, iters);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        printf("%s time %-14s %.3f us each (%d dependent calls, one wave)\n", name, what[mode], ms * 1000.0f / iters, iters);
    }
    hipFree(d_in);
    hipFree(d_ops);
    hipFree(d_l);
    hipFree(d_r);
    return bad;
}

int main() {
    int bad = run<alt_bn128_fq>("alt_bn128_fq");
    if (bad < 1000000) bad += run<bls12_377_fq>("bls12_377_fq");
    if (bad < 1000000) bad += run<bls12_381_fq>("bls12_381_fq");
    printf(bad ? "LAZY CHAIN TEST FAILED\n" : "LAZY CHAIN TEST PASSED\n");
    return bad ? 1 : 0;
}
