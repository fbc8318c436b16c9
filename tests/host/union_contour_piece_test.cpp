// Stand-alone run of tilingnn_amd/csrc/union_contour_piece.h -- the code the kernels of csrc/union_contour.hip run per tile and per
// piece -- on the host: reads tiles, contact rows and masks from a file, and per mask splits the sides, drops the twins, links the
// boundary pieces and walks the rings from their leaders, serially.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/union_contour_piece_test.cpp
// (tests/test_union_contour_host.py writes the file, builds and runs this, and compares with the loop-tracing oracle).
//
// File: int64 n_tiles, n_pts, n_touch, n_masks; double tol; then ring_xy [n_pts][2] f64, ring_ptr [n_tiles + 1] i32,
// touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, alive [n_masks][n_tiles] i32.
// Output per mask: "mask <pieces> <most splits on one side> <rings>", then per ring "ring <pts_src ...>"; at the end "err <bits>".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "union_contour_piece.h"

using namespace tgnn::contour;

template <class T>
static std::vector<T> read_array(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

struct CountSink {
    int n = 0;
    void operator()(int32_t, int32_t, int32_t) { ++n; }
};

struct FillSink {
    Pieces pc;
    int32_t at, tile;
    void operator()(int32_t side, int32_t src, int32_t end) {
        pc.tile[at] = tile;
        pc.side[at] = side;
        pc.src[at] = src;
        pc.end[at] = end;
        ++at;
    }
};

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = read_array<int64_t>(f, 4);
    const std::vector<double> par = read_array<double>(f, 1);
    const int64_t n = head[0], n_pts = head[1], n_touch = head[2], n_masks = head[3];
    const std::vector<double> ring_xy = read_array<double>(f, 2 * (size_t)n_pts);
    const std::vector<int32_t> ring_ptr = read_array<int32_t>(f, (size_t)n + 1), touch_ptr = read_array<int32_t>(f, (size_t)n + 1);
    const std::vector<int32_t> touch_idx = read_array<int32_t>(f, (size_t)n_touch);
    const std::vector<int32_t> alive = read_array<int32_t>(f, (size_t)n_masks * (size_t)n);
    fclose(f);
    const Tiles g{reinterpret_cast<const Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(), par[0], 1.0,
                  0.0};
    int err = 0;
    Splits sp;
    Leaving lv;
    for (int64_t k = 0; k < n_masks; ++k) {
        const int32_t *al = alive.data() + k * n;
        std::vector<int32_t> first((size_t)n + 1, 0);
        int most = 0;
        for (int64_t i = 0; i < n; ++i) {
            CountSink sink;
            if (al[i] != 0) {
                tile_pieces(g, al, i, sp, err, sink);
                const int32_t v0 = ring_ptr[i], m = ring_ptr[i + 1] - v0;
                for (int32_t s = 0; s < m; ++s) {
                    const Pt *r = g.ring_xy + v0;
                    side_splits(g, al, i, r[s], r[s + 1 == m ? 0 : s + 1], sp, err);
                    most = sp.n > most ? sp.n : most;
                }
            }
            first[(size_t)i + 1] = first[(size_t)i] + sink.n;
        }
        const int32_t pieces = first[(size_t)n];
        std::vector<int32_t> tile((size_t)pieces), side((size_t)pieces), src((size_t)pieces), end((size_t)pieces);
        std::vector<int32_t> next((size_t)pieces), seen((size_t)pieces, 0);
        const Pieces pc{tile.data(), side.data(), src.data(), end.data()};
        for (int64_t i = 0; i < n; ++i) {
            if (first[(size_t)i + 1] == first[(size_t)i]) continue;
            FillSink sink{pc, first[(size_t)i], (int32_t)i};
            tile_pieces(g, al, i, sp, err, sink);
            if (sink.at != first[(size_t)i + 1]) err |= kErrTrace;
        }
        bool broken = false;
        for (int32_t e = 0; e < pieces; ++e) {
            next[(size_t)e] = link_piece(g, al, first.data(), pc, e, lv, err);
            if (next[(size_t)e] < 0) broken = true;
            else ++seen[(size_t)next[(size_t)e]];
        }
        for (int32_t e = 0; e < pieces; ++e) broken |= seen[(size_t)e] != 1;
        if (broken) {
            err |= kErrTrace;
            printf("mask %d %d 0\n", pieces, most);
            continue;
        }
        std::vector<std::vector<int32_t>> rings;
        std::fill(seen.begin(), seen.end(), 0);
        for (int32_t lead = 0; lead < pieces; ++lead) {      // ascending: the first unseen piece of a cycle is its leader
            if (seen[(size_t)lead]) continue;
            rings.emplace_back();
            int32_t e = lead, before = -1;
            for (int32_t q = lead;; q = next[(size_t)q]) {   // the piece before the leader
                seen[(size_t)q] = 1;
                if (next[(size_t)q] == lead) {
                    before = q;
                    break;
                }
            }
            do {
                if (is_corner(g, pc, before, e)) rings.back().push_back(src[(size_t)e]);
                before = e;
                e = next[(size_t)e];
            } while (e != lead);
        }
        printf("mask %d %d %d\n", pieces, most, (int)rings.size());
        for (const auto &r : rings) {
            printf("ring");
            for (int32_t v : r) printf(" %d", v);
            printf("\n");
        }
    }
    printf("err %d\n", err);
    return 0;
}
