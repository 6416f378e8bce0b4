// Stand-alone check of libff_amd/csrc/write_plan.h, the chunk plan of amdmsm_write_points_stream / _file: walks the plan
// in the order write_impl (engine.cpp) does -- chunk k copied into staging buffer k % 2, then chunk k - 1 handed over --
// with the source, the two staging buffers and the written stream heap blocks of their exact sizes, and compares what was
// written with the source.  Meant for the host compiler's sanitizers (tests/test_keygen_output_cpu.py):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I libff_amd/csrc tools/write_plan_check.cpp -o check && ./check
// No HIP, no GPU.  Exit status 0 and "ok" when every case agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "write_plan.h"

using namespace amdmsm;

namespace {

int failures = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            printf("FAIL " __VA_ARGS__); \
            printf("\n");             \
            ++failures;               \
        }                             \
    } while (0)

void run(size_t n, size_t chunk_points, size_t rec) {
    const write_plan p = write_plan_of(n, chunk_points);
    CHECK(p.n == n, "n=%zu", n);
    if (!n) {
        CHECK(p.nchunks == 0, "n=0 chunk=%zu: %zu chunks", chunk_points, p.nchunks);
        return;
    }
    const size_t want_cp = chunk_points ? (chunk_points < n ? chunk_points : n) : (WRITE_DEFAULT_CHUNK < n ? WRITE_DEFAULT_CHUNK : n);
    CHECK(p.chunk_points == want_cp && p.nchunks == (n + want_cp - 1) / want_cp, "n=%zu chunk=%zu: plan %zu x %zu", n, chunk_points,
          p.nchunks, p.chunk_points);
    std::unique_ptr<unsigned char[]> src(new unsigned char[n * rec]), out(new unsigned char[n * rec]);
    std::unique_ptr<unsigned char[]> stage[WRITE_BUFFERS];
    bool full[WRITE_BUFFERS] = {};
    for (auto &s : stage) s.reset(new unsigned char[p.chunk_points * rec]);
    for (size_t i = 0; i < n * rec; ++i) src[i] = (unsigned char)(i * 2654435761u >> 13);
    memset(out.get(), 0xEE, n * rec);
    size_t written = 0;
    auto hand_over = [&](size_t k) {
        const write_chunk c = write_plan_chunk(p, k);
        CHECK(full[c.buffer], "n=%zu chunk=%zu: buffer of chunk %zu is empty", n, chunk_points, k);
        CHECK(c.first * rec == written, "n=%zu chunk=%zu: chunk %zu out of order", n, chunk_points, k);
        memcpy(out.get() + written, stage[c.buffer].get(), c.count * rec);
        written += c.count * rec;
        full[c.buffer] = false;
    };
    for (size_t k = 0; k < p.nchunks; ++k) {
        const write_chunk c = write_plan_chunk(p, k);
        CHECK(c.buffer >= 0 && c.buffer < WRITE_BUFFERS && c.count >= 1 && c.count <= p.chunk_points, "n=%zu chunk=%zu: chunk %zu",
              n, chunk_points, k);
        CHECK(!full[c.buffer], "n=%zu chunk=%zu: chunk %zu overwrites a buffer not handed over", n, chunk_points, k);
        memcpy(stage[c.buffer].get(), src.get() + c.first * rec, c.count * rec);
        full[c.buffer] = true;
        if (k) hand_over(k - 1);
    }
    hand_over(p.nchunks - 1);
    CHECK(written == n * rec && memcmp(out.get(), src.get(), n * rec) == 0, "n=%zu chunk=%zu: the stream differs from the source", n,
          chunk_points);
}

}   // namespace

int main() {
    const size_t sizes[] = {0, 1, 2, 5, 63, 64, 65, 128, 193, 1000};
    const size_t chunks[] = {0, 1, 2, 3, 64, 65, 1000, 4096};
    for (size_t n : sizes)
        for (size_t c : chunks)
            for (size_t rec : {(size_t)32, (size_t)80}) run(n, c, rec);
    run(((size_t)1 << 20) + 1, 0, 1);   // the default chunk, one record over
    run((size_t)3 << 20, 0, 1);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
