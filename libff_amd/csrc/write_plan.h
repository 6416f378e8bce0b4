// The chunk plan of the point writers (amdmsm_write_points_stream / _file, engine.cpp): n records leave the device
// chunk_points at a time through two staging buffers, chunk k through buffer k % 2.  Host-only and free of HIP, so that
// tools/write_plan_check.cpp can walk it under the host compiler's sanitizers.
#pragma once
#include <stddef.h>

namespace amdmsm {

constexpr size_t WRITE_DEFAULT_CHUNK = (size_t)1 << 20;   // the readers' default (stream_impl)
constexpr int WRITE_BUFFERS = 2;

struct write_plan {
    size_t n = 0, chunk_points = 0, nchunks = 0;
};
struct write_chunk {
    size_t first = 0, count = 0;
    int buffer = 0;
};

// chunk_points = 0: the default; never more than n, so that the staging buffers are no larger than the vector
inline write_plan write_plan_of(size_t n, size_t chunk_points) {
    write_plan p;
    p.n = n;
    p.chunk_points = chunk_points ? chunk_points : WRITE_DEFAULT_CHUNK;
    if (n && p.chunk_points > n) p.chunk_points = n;
    p.nchunks = n ? (n - 1) / p.chunk_points + 1 : 0;
    return p;
}
// chunk k < nchunks: records [first, first + count), count >= 1; the chunks follow one another and end at n
inline write_chunk write_plan_chunk(const write_plan &p, size_t k) {
    write_chunk c;
    c.first = k * p.chunk_points;
    c.count = p.n - c.first < p.chunk_points ? p.n - c.first : p.chunk_points;
    c.buffer = (int)(k % WRITE_BUFFERS);
    return c;
}

}   // namespace amdmsm
