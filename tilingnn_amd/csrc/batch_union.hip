// tgnn_batch_union: the disjoint union of B layouts out of a packed set (PyG's Batch.from_data_list for the four arrays the
// network and the loss read), in ONE launch.  A plain copy kernel: no LDS, no cross-lane step, no atomics -- every output
// element is written by exactly one thread from exactly one source element, so the bits are the same on every call.
//
// Work assignment: every output array is cut into 16-byte units (4 floats / 2 int64) of its FLAT element range; the four
// arrays' units follow each other in one index space the grid strides over.  A unit finds its owning member by a binary
// search in the output offset table; a unit that straddles members (or the two rows of an edge index) walks on from there.
// The store of a full unit is 16 bytes wide whenever the output array starts 16-byte aligned (torch allocations do); the load
// is 16 bytes wide when the unit lies in ONE member and its source address is 16-byte aligned (base and element) -- with 12-byte node
// rows most members start unaligned in source or destination, then four (two) scalar loads feed the wide store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tgnn.h"
#include "tgnn_common.h"

namespace tgnn {

static constexpr int kBuThreads = 256;

struct BatchUnionArgs {
    const float *x;            // packed [sum N][fx]
    const int64_t *adj;        // packed, layout k: [2][Ea_k] at element 2 * adj_ptr[k], local numbering
    const float *attr;         // packed [sum Ea][fe]
    const int64_t *col;        // packed like adj
    const int64_t *node_ptr, *adj_ptr, *col_ptr;     // [K + 1], device
    const int64_t *ids;        // [B]                 } one table on the device: ids | node_off | adj_off | col_off
    const int64_t *node_off, *adj_off, *col_off;     // [B + 1] each
    int32_t batch, fx, fe;
    int32_t wide;              // bit s: the SOURCE base of segment s (x, attr, adj, col) is 16-byte aligned (wide loads allowed);
                               // bit 4 + s: its DESTINATION base is (wide stores)
    float *x_out, *attr_out;
    int64_t *adj_out, *col_out;
    int64_t units_x, units_attr, units_adj, units_col;
};

// the member b with off[b] <= v < off[b + 1] (v < off[B]; empty members are passed over: the LAST b with off[b] <= v)
__host__ __device__ __forceinline__ int owner(const int64_t *off, int batch, int64_t v) {
    int lo = 0, hi = batch;                       // invariant: off[lo] <= v < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// rows of f floats: out[(off[b] + r) * f + c] = src[(src_ptr[ids[b]] + r) * f + c]
__host__ __device__ __forceinline__ void copy_rows_unit(const float *__restrict__ src, float *__restrict__ dst,
                                                        const int64_t *__restrict__ src_ptr, const int64_t *__restrict__ ids,
                                                        const int64_t *__restrict__ off, int batch, int64_t f, bool wide_ld, bool wide_st,
                                                        int64_t unit) {
    const int64_t total = off[batch] * f;
    const int64_t e0 = unit * 4;
    if (e0 >= total) return;
    int b = owner(off, batch, e0 / f);
    int64_t shift = (src_ptr[ids[b]] - off[b]) * f;          // source element = output element + shift, inside member b
    const bool full = e0 + 3 < total;
    float4 v;
    if (full && wide_ld && e0 + 3 < off[b + 1] * f && ((e0 + shift) & 3) == 0) {
        v = *reinterpret_cast<const float4 *>(src + e0 + shift);
    } else {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = e0 + j;
            if (e < total) {
                if (e >= off[b + 1] * f) {
                    do ++b; while (e >= off[b + 1] * f);      // (e < off[B] * f: ends at b <= B - 1)
                    shift = (src_ptr[ids[b]] - off[b]) * f;
                }
                t[j] = src[e + shift];
            }
        }
        v = make_float4(t[0], t[1], t[2], t[3]);
    }
    if (full && wide_st) {
        *reinterpret_cast<float4 *>(dst + e0) = v;
    } else {
        const float t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < total) dst[e0 + j] = t[j];
    }
}

// an edge index: out[r * E + off[b] + e] = src[2 * src_ptr[k] + r * E_k + e] + node_off[b],  k = ids[b], E = off[B], r = 0, 1
__host__ __device__ __forceinline__ void copy_index_unit(const int64_t *__restrict__ src, int64_t *__restrict__ dst,
                                                         const int64_t *__restrict__ src_ptr, const int64_t *__restrict__ ids,
                                                         const int64_t *__restrict__ off, const int64_t *__restrict__ node_off,
                                                         int batch, bool wide_ld, bool wide_st, int64_t unit) {
    const int64_t edges = off[batch], total = 2 * edges;
    const int64_t e0 = unit * 2;
    if (e0 >= total) return;
    const bool full = e0 + 1 < total;
    int64_t v[2] = {0, 0};
    bool loaded = false;
    {
        const int64_t r = e0 >= edges ? 1 : 0, g = e0 - r * edges;
        const int b = owner(off, batch, g);
        const int64_t k = ids[b], ek = off[b + 1] - off[b];
        const int64_t s = 2 * src_ptr[k] + r * ek + (g - off[b]);
        const int64_t add = node_off[b];
        if (full && wide_ld && g + 1 < off[b + 1] && (s & 1) == 0) {     // (g + 1 < off[b + 1] <= edges: the same row too)
            const longlong2 w = *reinterpret_cast<const longlong2 *>(src + s);
            v[0] = w.x + add;
            v[1] = w.y + add;
            loaded = true;
        } else {
            v[0] = src[s] + add;
        }
    }
    if (!loaded && full) {
        const int64_t e = e0 + 1;
        const int64_t r = e >= edges ? 1 : 0, g = e - r * edges;
        const int b = owner(off, batch, g);
        const int64_t ek = off[b + 1] - off[b];
        v[1] = src[2 * src_ptr[ids[b]] + r * ek + (g - off[b])] + node_off[b];
    }
    if (full && wide_st) {
        longlong2 w;
        w.x = v[0];
        w.y = v[1];
        *reinterpret_cast<longlong2 *>(dst + e0) = w;
    } else {
        dst[e0] = v[0];
        if (full) dst[e0 + 1] = v[1];
    }
}

__global__ __launch_bounds__(kBuThreads) void batch_union_kernel(BatchUnionArgs a) {
    const int64_t total = a.units_x + a.units_attr + a.units_adj + a.units_col;
    const int64_t stride = (int64_t)gridDim.x * kBuThreads;
    for (int64_t u = (int64_t)blockIdx.x * kBuThreads + threadIdx.x; u < total; u += stride) {
        int64_t w = u;
        if (w < a.units_x) {
            copy_rows_unit(a.x, a.x_out, a.node_ptr, a.ids, a.node_off, a.batch, a.fx, a.wide & 1, a.wide & 16, w);
            continue;
        }
        w -= a.units_x;
        if (w < a.units_attr) {
            copy_rows_unit(a.attr, a.attr_out, a.adj_ptr, a.ids, a.adj_off, a.batch, a.fe, a.wide & 2, a.wide & 32, w);
            continue;
        }
        w -= a.units_attr;
        if (w < a.units_adj) {
            copy_index_unit(a.adj, a.adj_out, a.adj_ptr, a.ids, a.adj_off, a.node_off, a.batch, a.wide & 4, a.wide & 64, w);
            continue;
        }
        w -= a.units_adj;
        copy_index_unit(a.col, a.col_out, a.col_ptr, a.ids, a.col_off, a.node_off, a.batch, a.wide & 8, a.wide & 128, w);
    }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace tgnn

using namespace tgnn;

extern "C" int tgnn_batch_union(const float *x, const int64_t *adj, const float *attr, const int64_t *col,
                                const int64_t *node_ptr, const int64_t *adj_ptr, const int64_t *col_ptr,
                                const int64_t *node_ptr_host, const int64_t *adj_ptr_host, const int64_t *col_ptr_host,
                                int32_t n_layouts, int32_t fx, int32_t fe, const int64_t *table_host, const int64_t *table,
                                int32_t batch, float *x_out, float *attr_out, int64_t *adj_out, int64_t *col_out,
                                tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_layouts >= 0 && batch >= 0 && fx >= 1 && fe >= 1, "shape");
    if (batch == 0) return TGNN_OK;
    TGNN_CHECK_ARG(n_layouts >= 1, "a batch out of an empty set");
    TGNN_CHECK_ARG(node_ptr_host && adj_ptr_host && col_ptr_host && table_host, "null host table");
    TGNN_CHECK_ARG(node_ptr && adj_ptr && col_ptr && table, "null device table");
    const int64_t *ids_h = table_host, *off_h[3] = {ids_h + batch, ids_h + 2 * (int64_t)batch + 1, ids_h + 3 * (int64_t)batch + 2};
    const int64_t *ptr_h[3] = {node_ptr_host, adj_ptr_host, col_ptr_host};
    static const char *const what[3] = {"node", "adjacency", "collision"};
    const int64_t cap = 1ll << 56;                           // (so that 4 * fx * N and 2 * E cannot wrap)
    for (int t = 0; t < 3; ++t) {
        if (ptr_h[t][0] != 0 || ptr_h[t][n_layouts] > cap || off_h[t][0] != 0) {
            set_error("tgnn_batch_union: invalid argument: the %s tables must start at 0 (and stay below 2^56)", what[t]);
            return TGNN_ERR_INVALID_ARG;
        }
    }
    for (int32_t b = 0; b < batch; ++b) {
        const int64_t k = ids_h[b];
        if (k < 0 || k >= n_layouts) {
            set_error("tgnn_batch_union: invalid argument: ids[%d] = %lld is outside [0, %d)", b, (long long)k, n_layouts);
            return TGNN_ERR_INVALID_ARG;
        }
        for (int t = 0; t < 3; ++t) {
            const int64_t have = off_h[t][b + 1] - off_h[t][b], want = ptr_h[t][k + 1] - ptr_h[t][k];
            if (want < 0 || have != want) {
                set_error("tgnn_batch_union: invalid argument: %s offset table: member %d (layout %lld) spans %lld, the layout "
                          "has %lld", what[t], b, (long long)k, (long long)have, (long long)want);
                return TGNN_ERR_INVALID_ARG;
            }
        }
    }
    const int64_t n = off_h[0][batch], ea = off_h[1][batch], ec = off_h[2][batch];
    TGNN_CHECK_ARG(n <= cap / fx && ea <= cap / fe, "the union overflows");
    TGNN_CHECK_ARG((n == 0 || (x && x_out)) && (ea == 0 || (adj && attr && adj_out && attr_out)) && (ec == 0 || (col && col_out)),
                   "null array of a non-empty kind");
    BatchUnionArgs a;
    a.x = x, a.adj = adj, a.attr = attr, a.col = col;
    a.node_ptr = node_ptr, a.adj_ptr = adj_ptr, a.col_ptr = col_ptr;
    a.ids = table, a.node_off = table + batch, a.adj_off = table + 2 * (int64_t)batch + 1, a.col_off = table + 3 * (int64_t)batch + 2;
    a.batch = batch, a.fx = fx, a.fe = fe;
    a.wide = (aligned16(x) ? 1 : 0) | (aligned16(attr) ? 2 : 0) | (aligned16(adj) ? 4 : 0) | (aligned16(col) ? 8 : 0) |
             (aligned16(x_out) ? 16 : 0) | (aligned16(attr_out) ? 32 : 0) | (aligned16(adj_out) ? 64 : 0) | (aligned16(col_out) ? 128 : 0);
    a.x_out = x_out, a.attr_out = attr_out, a.adj_out = adj_out, a.col_out = col_out;
    a.units_x = (n * fx + 3) / 4, a.units_attr = (ea * fe + 3) / 4, a.units_adj = ea, a.units_col = ec;   // (2 E int64 = E units)
    const int64_t units = a.units_x + a.units_attr + a.units_adj + a.units_col;
    if (units == 0) return TGNN_OK;
    const int64_t blocks = (units + kBuThreads - 1) / kBuThreads;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);      // (16 blocks of 256 per CU; the rest by the stride loop)
    batch_union_kernel<<<grid, kBuThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
