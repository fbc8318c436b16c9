// Host-side plan of the fused Adam step (adam.hip: tgnn_adam_step): the segment table, the chunk list cut from it and the checks
// both get before a launch may read them.  Plain C++, no HIP header: tests/host/adam_plan_test.cpp compiles it with the host
// compiler alone.
//
//   segment = one parameter tensor: where the parameter lives, where its gradient sits RELATIVE to a base pointer that travels
//             as a kernel argument (bytes: gradients from torch's autograd are separate allocations, any distance apart), where
//             its two moments sit in the flat moment buffers (floats, 64-float = 256-byte aligned slices), how many elements.
//   chunk   = (segment, start): the elements [start, min(start + kAdamChunk, numel)) of that segment -- one block's work.  Starts
//             are multiples of kAdamChunk, so a chunk is 16-byte aligned exactly when its segment is.
//
// The table image the kernel reads is the segments followed by the chunks (adam_table_bytes); the same bytes are kept on the
// host, where tgnn_adam_step checks them before every launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tgnn {

constexpr int64_t kAdamChunk = 4096;          // elements per chunk: 256 threads x 4 x float4
constexpr int64_t kAdamMomentAlign = 64;      // floats: the moment slices start on 256-byte boundaries

struct AdamSegment {
    float *param;
    int64_t grad_off;      // BYTES from the launch's gradient base to this segment's gradient (a multiple of 4, any sign)
    int64_t moment_off;    // FLOATS into exp_avg / exp_avg_sq
    int64_t numel;
};
struct AdamChunk {
    int64_t start;         // first element inside the segment
    int32_t segment;
    int32_t reserved_;     // 0
};
static_assert(sizeof(AdamSegment) == 32 && sizeof(AdamChunk) == 16, "the table image's layout");

constexpr int64_t adam_chunks_of(int64_t numel) { return numel <= 0 ? 0 : (numel - 1) / kAdamChunk + 1; }

// moment slices of tensors laid out one after the other: offset of the next slice behind one of `numel` floats at `off`
constexpr int64_t adam_next_moment_off(int64_t off, int64_t numel) {
    return off + (numel + kAdamMomentAlign - 1) / kAdamMomentAlign * kAdamMomentAlign;
}

// chunks of all segments together, -1: a negative element count (or more chunks than a grid's x dimension holds)
inline int64_t adam_chunk_count(const int64_t *numel, int32_t n_segments) {
    if (n_segments < 0 || (n_segments > 0 && !numel)) return -1;
    int64_t total = 0;
    for (int32_t s = 0; s < n_segments; ++s) {
        if (numel[s] < 0) return -1;
        total += adam_chunks_of(numel[s]);
        if (total > (int64_t)0x7fffffff) return -1;
    }
    return total;
}

constexpr size_t adam_table_bytes(int32_t n_segments, int64_t n_chunks) {
    return (size_t)(n_segments < 0 ? 0 : n_segments) * sizeof(AdamSegment) + (size_t)(n_chunks < 0 ? 0 : n_chunks) * sizeof(AdamChunk);
}
inline const AdamChunk *adam_table_chunks(const void *table, int32_t n_segments) {
    return reinterpret_cast<const AdamChunk *>(static_cast<const char *>(table) + (size_t)n_segments * sizeof(AdamSegment));
}

// Writes the chunk list of `segs`, segment by segment in ascending starts; returns the number written (== adam_chunk_count).
inline int64_t adam_cut_chunks(const AdamSegment *segs, int32_t n_segments, AdamChunk *out) {
    int64_t k = 0;
    for (int32_t s = 0; s < n_segments; ++s)
        for (int64_t at = 0; at < segs[s].numel; at += kAdamChunk) out[k++] = AdamChunk{at, s, 0};
    return k;
}

// What a launch relies on, checked on the host image.  NULL = fine, else what is wrong (a static string).
inline const char *adam_check_segments(const AdamSegment *segs, int32_t n_segments, int64_t moment_floats) {
    if (n_segments < 0 || moment_floats < 0) return "negative count";
    for (int32_t s = 0; s < n_segments; ++s) {
        const AdamSegment &g = segs[s];
        if (g.numel < 0) return "negative element count";
        if (g.numel > 0 && !g.param) return "null parameter pointer";
        if (g.grad_off % 4 != 0) return "gradient offset is not a multiple of 4 bytes";
        if (g.moment_off < 0 || g.moment_off % kAdamMomentAlign != 0) return "moment offset is negative or not 64-float aligned";
        if (g.numel > moment_floats || g.moment_off > moment_floats - g.numel) return "moment slice ends outside the moment buffers";
    }
    return nullptr;
}
inline const char *adam_check_chunks(const AdamSegment *segs, int32_t n_segments, const AdamChunk *chunks, int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > (int64_t)0x7fffffff) return "chunk count out of range";
    for (int64_t k = 0; k < n_chunks; ++k) {
        const AdamChunk &c = chunks[k];
        if (c.segment < 0 || c.segment >= n_segments) return "chunk names a segment outside the table";
        if (c.start < 0 || c.start >= segs[c.segment].numel) return "chunk starts outside its segment";
        if (c.start % kAdamChunk != 0) return "chunk start is not a multiple of the chunk size";
    }
    return nullptr;
}

}  // namespace tgnn
