// Topology of the union of a set of tiles that do not overlap -- what the reference's `BrickLayout.detect_holes` asks of a solved
// layout (tiling/brick_layout.py:229-240: grow every selected tile by 1e-7, unary_union, look for interior rings) -- for K tile
// masks of the complete graph in one call: per mask the number of connected components of the CLOSED union of the alive tiles
// (tiles sharing any point, a single corner included, are connected) and the number of bounded components of its complement
// (holes; a gap sealed only by a corner-to-corner contact is one).
//
// Inputs: the rings and the collision CSR of csrc/union_area.hip, and the CONTACT CSR of tilingnn_amd/tiling/region.py:
// contact_geometry (row i = the tiles with a vertex within tol of tile i's ring, or the other way round).
//
// Formulation: Euler's relation chi = components - holes.  chi is a sum of local integer terms, one per distinct vertex position
// (union_topology_point.h: 1 - the number of arcs of the union just below the point, along a sweep direction no tile side is
// parallel to); only `components` needs global work.  A mask in which two alive tiles collide is outside that reasoning: it gets
// status 1 and counts of -1 (the collision CSR decides), never a guess.
//
// Launch shape.  union_topology_chi_kernel: grid (ceil(n_tiles / 128), K), a block per 128 tiles of one mask -- the shape of
// union_area_tiles_kernel with half the block, because a point's arcs live in LDS: 128 threads x 16 arcs x 16 B = 32 KB per
// block, laid out [slot][thread] (conflict free), 4 blocks per CU (256 threads would take the whole 64 KB a block may have and
// leave 2).  First ONE THREAD per tile: a dead tile costs one coalesced 4-byte load; an alive one scans its collision row and
// enters the block's list.  Then ONE THREAD per (listed tile, vertex): a solution has a fifth of the tiles alive, so threads per
// tile would leave four lanes in five idle through the whole of the work; the points fill them.  Each thread adds its integer
// terms to the mask's chi with one integer atomic: integer addition commutes, so every call gives the same bits.
// union_topology_fold_kernel: ONE BLOCK per mask labels the components by min-label propagation over the contact rows filtered
// by the mask, with pointer jumping, until a block-wide flag stays down (no grid barrier; union_masks.h: label_components, which
// csrc/union_hole_delta.hip and csrc/union_contour.hip run too); labels live in LDS for graphs of up to 6 144 tiles, in the
// caller's workspace beyond; components = alive tiles that kept their own index.  The memset of the K chi / status words and the
// two kernels follow each other on the stream; nothing returns to the host.
#include "union_masks.h"

namespace tgnn {

constexpr int kUtThreads = 128;
constexpr int kUtFoldThreads = 256;

struct TopoArgs : MaskSet {
    int32_t *label;                          // [K][n_tiles]   (workspace)
    int32_t *chi;                            // [K]            (workspace, zeroed per call)
    int32_t *status;                         // [K]            (workspace, zeroed per call)
    int32_t *out;                            // [K][3]
};

__global__ __launch_bounds__(kUtThreads) void union_topology_chi_kernel(TopoArgs a, int64_t mask0) {
    __shared__ double arc_lo[topo::kMaxWedges][kUtThreads], arc_hi[topo::kMaxWedges][kUtThreads];
    __shared__ int list[kUtThreads];
    __shared__ int n_list, max_verts;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kUtThreads + tid;
    const int64_t k = mask0 + blockIdx.y;
    const int32_t *al = a.alive + k * a.g.n_tiles;
    if (tid == 0) n_list = max_verts = 0;
    __syncthreads();
    int err = 0;
    // 1. one thread per tile: the collision rows, and the block's alive tiles into a list (in any order: the sum is of integers)
    if (i < a.g.n_tiles && al[i] != 0) {
        const int n = a.g.ring_ptr[i + 1] - a.g.ring_ptr[i];
        if (topo::collides(a.col_ptr, a.col_idx, al, i, a.g.n_tiles, 0, 1, err)) {
            atomicOr(a.status + k, 1);
        } else if (n >= 3) {
            list[atomicAdd(&n_list, 1)] = tid;
            atomicMax(&max_verts, n);
        }
    }
    __syncthreads();
    // 2. one thread per (alive tile, vertex): the alive tiles are few, so the points, not the tiles, fill the lanes
    const int tiles = n_list, points = tiles * max_verts;
    LdsArcs<kUtThreads> arcs{arc_lo, arc_hi, tid};
    int sum = 0;
    for (int w = tid; w < points; w += kUtThreads) {
        const int64_t t = (int64_t)blockIdx.x * kUtThreads + list[w % tiles];
        const int v = w / tiles;
        if (v < a.g.ring_ptr[t + 1] - a.g.ring_ptr[t]) sum += topo::point_term(a.g, al, t, v, arcs, err);
    }
    if (sum != 0) atomicAdd(a.chi + k, sum);
    if (err != 0) atomicOr(a.err_flag, err);
}

// kInLds: the labels and the list of the mask's alive tiles live in LDS (2 n_tiles words of dynamic LDS) and a round visits the
// alive tiles only; otherwise the labels live in the workspace and a round strides over all tiles (union_masks.h:
// label_components runs the rounds).  A label is -1 for a dead tile, else the index of an alive tile of the same component.
template <bool kInLds>
__global__ __launch_bounds__(kUtFoldThreads) void union_topology_fold_kernel(TopoArgs a, int64_t mask0) {
    extern __shared__ int32_t fold_lds[];
    __shared__ int changed, roots, n_alive;
    const int tid = threadIdx.x;
    const int64_t k = mask0 + blockIdx.x;
    const int n = (int)a.g.n_tiles;
    const int32_t *al = a.alive + k * a.g.n_tiles;
    volatile int32_t *lab = kInLds ? fold_lds : a.label + k * a.g.n_tiles;
    int32_t *list = fold_lds + n;                            // (kInLds only)
    if (tid == 0) roots = n_alive = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kUtFoldThreads) {
        const bool alive = al[i] != 0;
        lab[i] = alive ? i : -1;
        if (kInLds && alive) list[atomicAdd(&n_alive, 1)] = i;
    }
    int err = 0;
    label_components<kUtFoldThreads, kInLds>(a.g, lab, list, &n_alive, &changed, err);
    int mine = 0;
    for (int i = tid; i < n; i += kUtFoldThreads) mine += lab[i] == i ? 1 : 0;
    if (mine != 0) atomicAdd(&roots, mine);
    if (err != 0) atomicOr(a.err_flag, err);
    __syncthreads();
    if (tid == 0) {
        const bool bad = a.status[k] != 0;
        a.out[3 * k + 0] = bad ? -1 : roots;
        a.out[3 * k + 1] = bad ? -1 : roots - a.chi[k];
        a.out[3 * k + 2] = bad ? 1 : 0;
    }
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_union_topology_workspace_bytes(int64_t n_masks, int64_t n_tiles) {
    if (n_masks <= 0 || n_tiles <= 0 || n_masks > (1ll << 58) / (n_tiles + 2)) return 0;
    return (size_t)n_masks * ((size_t)n_tiles + 2) * sizeof(int32_t);
}

extern "C" int tgnn_union_topology(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *col_ptr,
                                   const int32_t *col_idx, const int32_t *touch_ptr, const int32_t *touch_idx,
                                   const int32_t *alive, int64_t n_masks, double tol, double dir_x, double dir_y, int32_t *out,
                                   int32_t *err_flag, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (int rc = check_mask_shape(__func__, n_tiles, n_masks, tol, dir_x, dir_y)) return rc;
    if (n_masks == 0) return TGNN_OK;
    TGNN_CHECK_ARG(out && err_flag, "null out / err_flag");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_tiles == 0) {
        TGNN_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(int32_t) * 3 * n_masks, s));
        return TGNN_OK;
    }
    if (int rc = check_mask_arrays(__func__, n_masks, (1ll << 58) / (n_tiles + 2), ring_xy && ring_ptr && col_ptr && touch_ptr && alive,
                                   ws, ws_bytes, tgnn_union_topology_workspace_bytes(n_masks, n_tiles), sizeof(int32_t)))
        return rc;
    int32_t *words = static_cast<int32_t *>(ws);
    TopoArgs a{{{reinterpret_cast<const topo::Pt *>(ring_xy), ring_ptr, n_tiles, touch_ptr, touch_idx, tol, dir_x, dir_y},
                col_ptr, col_idx, alive, n_masks, err_flag},
               words + 2 * n_masks, words, words + n_masks, out};
    TGNN_CHECK_HIP(hipMemsetAsync(words, 0, sizeof(int32_t) * 2 * n_masks, s));
    const unsigned gx = (unsigned)((n_tiles + kUtThreads - 1) / kUtThreads);
    for_mask_chunks(n_masks, kMaskGridY, [&](int64_t k0, unsigned gy) {
        union_topology_chi_kernel<<<dim3(gx, gy), kUtThreads, 0, s>>>(a, k0);
    });
    for_mask_chunks(n_masks, kMaskGridX, [&](int64_t k0, unsigned g) {
        if (n_tiles <= kLabelLdsTiles)
            union_topology_fold_kernel<true><<<g, kUtFoldThreads, 2 * sizeof(int32_t) * n_tiles, s>>>(a, k0);
        else
            union_topology_fold_kernel<false><<<g, kUtFoldThreads, 0, s>>>(a, k0);
    });
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
