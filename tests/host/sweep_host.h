// What the two stand-alone walk programs share (hole_sweep_step_test.cpp, tree_sweep_step_test.cpp): the case file, the state of
// ONE layout with node i = tile i, and the acceptance of a node by one worker from the sweep:: steps of
// tilingnn_amd/csrc/hole_sweep_step.h -- what block_accept (csrc/hole_sweep_block.h) shares among a block's threads -- with the
// check of the label invariant behind it.  The visit rule, the counters of a round and the output rows are each program's own.
//
// File: int64 head [n_head] = n_tiles, n_pts, n_touch, n_nbr, n_orders and the program's further words; double tol, dir_x, dir_y;
// then ring_xy [n_pts][2] f64, ring_ptr [n_tiles + 1] i32, touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, nbr_ptr
// [n_tiles + 1] i32, nbr_idx [n_nbr] i32 (scripted "collision" rows: what an acceptance labels), want [2^n_tiles][2] i32 =
// (components, holes) of every subset, rate [n_tiles] f64 by position (thr or p), orders [n_orders][n_tiles] u8.
// Draw j of order o is ((7 o + 13 j) mod 32) / 32.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hole_sweep_step.h"

using namespace tgnn;

struct HostArcs {
    double lo_[topo::kMaxWedges], hi_[topo::kMaxWedges];
    double &lo(int q) { return lo_[q]; }
    double &hi(int q) { return hi_[q]; }
};

template <class T>
static std::vector<T> read_array(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

static int32_t find(std::vector<int32_t> &parent, int32_t a) {
    while (parent[a] != a) a = parent[a] = parent[parent[a]];
    return a;
}

static double scripted_draw(int64_t order, int draws) { return (double)((7 * order + 13 * draws) % 32) / 32.0; }

struct HostWalk {
    std::vector<int64_t> head;
    std::vector<double> par, ring_xy, rate;
    std::vector<int32_t> ring_ptr, touch_ptr, touch_idx, nbr_ptr, nbr_idx, want;
    std::vector<uint8_t> orders;
    int64_t n = 0, n_orders = 0;
    topo::Tiles g{};
    HostArcs arcs;
    // the state of the order that is being walked, and what every order adds to
    std::vector<int32_t> alive, label, chi, unl, parent;
    int mask = 0, accepted = 0, killed = 0;
    int err = 0;
    long mismatches = 0;

    // Exits with status 2 on a file that is not one.
    HostWalk(const char *path, size_t n_head) {
        FILE *f = fopen(path, "rb");
        if (!f) exit(2);
        head = read_array<int64_t>(f, n_head);
        par = read_array<double>(f, 3);
        n = head[0], n_orders = head[4];
        if (n < 1 || n > 16) exit(2);
        ring_xy = read_array<double>(f, 2 * (size_t)head[1]);
        ring_ptr = read_array<int32_t>(f, (size_t)n + 1), touch_ptr = read_array<int32_t>(f, (size_t)n + 1);
        touch_idx = read_array<int32_t>(f, (size_t)head[2]);
        nbr_ptr = read_array<int32_t>(f, (size_t)n + 1), nbr_idx = read_array<int32_t>(f, (size_t)head[3]);
        want = read_array<int32_t>(f, 2 * ((size_t)1 << n));
        rate = read_array<double>(f, (size_t)n);
        orders = read_array<uint8_t>(f, (size_t)n_orders * (size_t)n);
        fclose(f);
        g = topo::Tiles{reinterpret_cast<const topo::Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(),
                        par[0], par[1], par[2]};
        alive.resize((size_t)n), label.resize((size_t)n), chi.resize((size_t)n), unl.resize((size_t)n), parent.resize((size_t)n);
    }

    void reset() {
        for (int64_t i = 0; i < n; ++i) alive[i] = 0, label[i] = -1, unl[i] = 1, chi[i] = sweep::kChiUnknown;
        mask = accepted = killed = 0;
    }

    // d holes the subset table gives for tile t on the present selection, against the walk's d.
    void check_delta(int d, int64_t o, int64_t pos, int64_t t) {
        const int expect = want[2 * (mask | 1 << t) + 1] - want[2 * mask + 1];
        if (d != expect && ++mismatches <= 10)
            fprintf(stderr, "order %ld position %ld: selection %#x tile %ld: d holes %d, expected %d\n", (long)o, (long)pos, mask, (long)t,
                    d, expect);
    }

    // Accepts `node` (= its tile) at position pos of order o: the merge, the label invariant, then the node's collision row.
    // room: the nodes the killed list may hold once the node is accepted (a mismatch when a kill does not fit).
    void accept(int64_t o, int64_t pos, int64_t node, int64_t room) {
        const int64_t t = node;
        unl[node] = 0;
        ++accepted;
        int32_t m = sweep::begin_merge(alive.data(), label.data(), t);
        for (int cc = touch_ptr[t]; cc < touch_ptr[t + 1]; ++cc) {
            const int32_t root = sweep::mark_root(g, label.data(), t, cc, err);
            m = root < m ? root : m;
            sweep::forget_chi(g, chi.data(), cc, err);
        }
        for (int64_t i = 0; i < n; ++i) sweep::join_member(label.data(), n, i, m);
        for (int64_t i = 0; i < n; ++i) sweep::close_root(label.data(), i, m);
        mask |= 1 << t;
        // the label invariant: -1 for a dead tile, else the lowest alive tile of its component
        for (int32_t i = 0; i < n; ++i) parent[i] = i;
        for (int32_t i = 0; i < n; ++i) {
            if (alive[i] == 0) continue;
            for (int cc = touch_ptr[i]; cc < touch_ptr[i + 1]; ++cc) {
                const int32_t j = touch_idx[cc];
                if (alive[j] == 0) continue;
                const int32_t a = find(parent, i), b = find(parent, j);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;
            }
        }
        for (int32_t i = 0; i < n; ++i) {
            const int32_t expect_label = (mask >> i & 1) ? find(parent, i) : -1;
            if ((alive[i] != 0) != ((mask >> i & 1) != 0) || label[i] != expect_label) {
                if (++mismatches <= 10)
                    fprintf(stderr, "order %ld position %ld: selection %#x: label[%d] = %d, expected %d\n", (long)o, (long)pos, mask, i,
                            label[i], expect_label);
            }
        }
        for (int64_t cc = nbr_ptr[node]; cc < nbr_ptr[node + 1]; ++cc) {
            const int32_t v = sweep::killed_by(nbr_idx.data(), nbr_ptr[node], cc, unl.data(), n, err);
            if (v < 0) continue;
            if (killed + 1 > room) ++mismatches;
            unl[v] = 0;
            ++killed;
        }
    }

    // Writes the programs' rows; false when the file cannot be written.
    static bool write_rows(const char *path, const std::vector<int32_t> &out) {
        FILE *w = fopen(path, "wb");
        if (!w || fwrite(out.data(), sizeof(int32_t), out.size(), w) != out.size()) return false;
        fclose(w);
        return true;
    }
};
