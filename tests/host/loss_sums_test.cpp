// Stand-alone run of tilingnn_amd/csrc/loss_sums.h and many_desc.h -- the planning, lookup and per-thread arithmetic that the
// single-layout and the K-layout loss and score kernels share -- on the host.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/loss_sums_test.cpp
// (tests/test_loss_many_host.py builds and runs this.)
//
// 4 000 random packed sets (empty members, empty edge sets, sub-layout counts, inactive members), exact-size heap buffers, and
// offset tables / counts / edge ends that are broken on purpose in every third trial.  Every (layout, block, thread) of the launch
// geometry is walked, for the loss sums and for the score sums; a layout the view rejects must be exactly a broken one, every
// other layout's sums are compared with a plain loop.  Before that: loss_blocks at the sizes where the count changes, in each
// position, and the final formula against its three factors written out.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "loss_sums.h"

using namespace tgnn;
template <typename T> static T *exact(size_t count) {               // exact-size heap block: one element past it is a report
    void *p = malloc(count ? count * sizeof(T) : 1);
    if (!p) abort();
    return static_cast<T *>(p);
}
static int check_blocks_and_formula() {
    const int64_t items[] = {0, 1, 1024, 1025, 524288, 524289};
    const int want[] = {1, 1, 1, 2, 512, 512};
    for (int q = 0; q < 6; ++q) {
        const int64_t big = items[q], small = big < 3 ? big : 3;
        if (loss_blocks(big, small, small) != want[q] || loss_blocks(small, big, small) != want[q] || loss_blocks(small, small, big) != want[q]) {
            printf("loss_blocks at %lld items: want %d\n", (long long)big, want[q]);
            return 1;
        }
    }
    const double s[3] = {12.5, -40.0, -7.0};
    double t[3];
    const double l = loss_from_sums(s, 50, 20, 0, 0.5f, 2.0f, 0.25f, t);
    if (t[0] != log(0.25) || t[1] != -2.0 || t[2] != 0.0 || fabs(l - (1.0 - 0.25 * t[0]) * (1.0 - 0.5 * t[1])) > 1e-15 * l) { printf("formula\n"); return 1; }
    const double z[3] = {0.0, 0.0, 0.0};
    loss_from_sums(z, 5, 0, 0, 1.f, 1.f, 1.f, t);
    if (t[0] != log((double)kLossEps) || t[1] != 0.0) { printf("formula at the floor\n"); return 1; }
    return 0;
}
int main() {
    if (check_blocks_and_formula()) return 1;
    std::mt19937_64 rng(1);
    long layouts_walked = 0, rejected = 0, edges_skipped = 0, score_edges_skipped = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        const int K = 1 + rng() % 7, M = 1 + rng() % 3, ldp = M + rng() % 2, lda = 1 + rng() % 3, ldl = 1 + rng() % 3;
        std::vector<int64_t> ptr[3];
        for (auto &p : ptr) p.assign(K + 1, 0);
        const int64_t max_size[3] = {40, 2600, 1500};
        for (int k = 0; k < K; ++k)
            for (int s = 0; s < 3; ++s) ptr[s][k + 1] = ptr[s][k] + (rng() % 4 == 0 ? 0 : rng() % max_size[s]);
        const int64_t total[3] = {ptr[0][K], ptr[1][K], ptr[2][K]};
        const bool with_counts = trial % 2 == 1, with_active = trial % 5 == 0, broken = trial % 3 == 0;
        std::vector<int64_t> counts(3 * K);
        std::vector<int32_t> active(K);
        for (int k = 0; k < K; ++k) {
            active[k] = rng() % 4 != 0;
            for (int s = 0; s < 3; ++s) counts[3 * k + s] = rng() % (ptr[s][k + 1] - ptr[s][k] + 1);
        }
        // the buffers: exact sizes
        float *area = exact<float>(total[0] * lda), *len = exact<float>(total[1] * ldl);
        float *predict = exact<float>(total[0]), *perim = exact<float>(total[0]);
        int64_t *adj = exact<int64_t>(2 * total[1]), *col = exact<int64_t>(2 * total[2]);
        for (int64_t i = 0; i < total[0] * lda; ++i) area[i] = (float)(1 + rng() % 1000) / 1000.f;
        for (int64_t i = 0; i < total[1] * ldl; ++i) len[i] = (float)(1 + rng() % 1000) / 1000.f;
        for (int64_t i = 0; i < total[0]; ++i) {
            predict[i] = rng() % 3 == 0 ? 1.0f : (rng() % 2 ? 0.0f : (float)(rng() % 1000) / 1000.f);
            perim[i] = (float)(1 + rng() % 1000) / 100.f;
        }
        std::vector<float *> probs(K);
        auto size_of = [&](int s, int k) { return with_counts ? counts[3 * k + s] : ptr[s][k + 1] - ptr[s][k]; };
        for (int k = 0; k < K; ++k) {
            const int64_t n = size_of(0, k), ea = size_of(1, k), ec = size_of(2, k);
            probs[k] = exact<float>(n * ldp);
            for (int64_t i = 0; i < n * ldp; ++i) probs[k][i] = 0.01f + 0.98f * (float)(rng() % 1000) / 1000.f;
            for (int64_t e = 0; e < 2 * ea; ++e) adj[2 * ptr[1][k] + e] = n ? rng() % n : 0;
            for (int64_t e = 0; e < 2 * ec; ++e) col[2 * ptr[2][k] + e] = n ? rng() % n : 0;
            for (int64_t e = 2 * ea; e < 2 * (ptr[1][k + 1] - ptr[1][k]); ++e) adj[2 * ptr[1][k] + e] = -1 - (int64_t)(rng() % 1000);
            for (int64_t e = 2 * ec; e < 2 * (ptr[2][k + 1] - ptr[2][k]); ++e) col[2 * ptr[2][k] + e] = 1000000 + rng() % 1000;
        }
        // break something: an offset (negative, past the total, not monotonic), a count, or an edge end (the layout's own node
        // count: a valid row of the NEXT layout's probabilities, never of this one's)
        std::vector<char> bad_edge(K, 0);           // bad_edge: 1 = an adjacency end, 2 = a collision end
        std::vector<int64_t> tab[3] = {ptr[0], ptr[1], ptr[2]};
        if (broken) {
            const int k = rng() % K, s = rng() % 3;
            switch (rng() % 5) {
            case 0: tab[s][k] = -1 - (int64_t)(rng() % 5); break;
            case 1: tab[s][k + 1] = total[s] + 1 + rng() % 5; break;
            case 2: if (k + 1 < K) tab[s][k + 1] = tab[s][k] - 1 - (int64_t)(rng() % 3); break;
            case 3: if (with_counts) counts[3 * k + s] = (rng() % 2) ? -1 : ptr[s][k + 1] - ptr[s][k] + 1; break;
            default: {
                const int64_t n = size_of(0, k), e = size_of(s ? s : 1, k);
                int64_t *ei = (s == 2 ? col + 2 * ptr[2][k] : adj + 2 * ptr[1][k]);
                if (n && e) { ei[rng() % (2 * e)] = (rng() % 2) ? n : -1; bad_edge[k] = s == 2 ? 2 : 1; }
            } }
        }
        ManyDesc d{K, {tab[0].data(), tab[1].data(), tab[2].data()}, {total[0], total[1], total[2]},
                   with_active ? active.data() : nullptr, with_counts ? counts.data() : nullptr};
        for (int k = 0; k < K; ++k) {
            // what the definition says about layout k, from the tables as given
            bool want_bad = false;
            int64_t sz[3] = {0, 0, 0};
            const bool skipped = with_active && !active[k];
            for (int s = 0; s < 3 && !skipped; ++s) {
                const int64_t a = tab[s][k], b = tab[s][k + 1];
                if (a < 0 || b < a || b > total[s]) { want_bad = true; break; }
                sz[s] = b - a;
                if (with_counts) { if (counts[3 * k + s] < 0 || counts[3 * k + s] > sz[s]) { want_bad = true; break; } sz[s] = counts[3 * k + s]; }
            }
            LossManyView v;
            bool bad;
            const bool live = loss_many_view(d, k, v, bad);
            if (bad != want_bad) { printf("trial %d layout %d: bad %d, want %d\n", trial, k, bad, want_bad); return 1; }
            if (skipped || want_bad || sz[0] == 0) {
                if (live) { printf("trial %d layout %d: a view of nothing\n", trial, k); return 1; }
                rejected += want_bad;
                continue;
            }
            if (!live || v.n != sz[0] || v.ea != sz[1] || v.ec != sz[2]) { printf("trial %d layout %d: sizes\n", trial, k); return 1; }
            // a table broken for a neighbour may have moved this layout: its arrays are then somebody else's, still inside the buffers
            const bool moved = v.np != ptr[0][k] || v.ap != ptr[1][k] || v.cp != ptr[2][k] ||
                               (!with_counts && (v.n != ptr[0][k + 1] - ptr[0][k] || v.ea != ptr[1][k + 1] - ptr[1][k] ||
                                                 v.ec != ptr[2][k + 1] - ptr[2][k]));
            if (moved) continue;                                      // (its probabilities have the rows of the true size only)
            const int nb = loss_blocks(v.n, v.ec, v.ea);
            const int want_nb = (int)std::min<int64_t>(std::max<int64_t>((std::max(std::max(v.n, v.ec), v.ea) + 1023) / 1024, 1), 512);
            if (nb != want_nb) { printf("trial %d layout %d: %d blocks, want %d\n", trial, k, nb, want_nb); return 1; }
            for (int m = 0; m < M; ++m) {
                double s[3] = {0, 0, 0};
                bool edge_bad = false;
                for (int bl = 0; bl < nb; ++bl)
                    for (int t = 0; t < kMnThreads; ++t)
                        loss_accumulate(v.n, v.ec, v.ea, probs[k] + m, ldp, area + v.np * lda, lda, col + 2 * v.cp, adj + 2 * v.ap,
                                        len + v.ap * ldl, ldl, (int64_t)bl * kMnThreads + t, (int64_t)nb * kMnThreads, s[0], s[1], s[2],
                                        edge_bad);
                if (edge_bad != (bool)bad_edge[k]) { printf("trial %d layout %d: edge report %d\n", trial, k, edge_bad); return 1; }
                edges_skipped += edge_bad;
                if (edge_bad) continue;
                double w[3] = {0, 0, 0};
                const float *p = probs[k] + m;
                for (int64_t i = 0; i < v.n; ++i) w[0] += (double)(area[(v.np + i) * lda] * p[i * ldp]);
                for (int64_t e = 0; e < v.ec; ++e) {
                    float pp = p[col[2 * v.cp + e] * ldp] * p[col[2 * v.cp + v.ec + e] * ldp];
                    w[1] += (double)logf(1.0f - fminf(fmaxf(pp, 1e-7f), 1.0f - 1e-7f));
                }
                for (int64_t e = 0; e < v.ea; ++e) {
                    float pp = p[adj[2 * v.ap + e] * ldp] * p[adj[2 * v.ap + v.ea + e] * ldp] * len[(v.ap + e) * ldl];
                    w[2] += (double)(logf(fmaxf(pp, 1e-7f)) / 2.302585092994046f);
                }
                for (int c = 0; c < 3; ++c)
                    if (fabs(s[c] - w[c]) > 1e-9 * (1.0 + fabs(w[c]))) { printf("trial %d layout %d sum %d: %g vs %g\n", trial, k, c, s[c], w[c]); return 1; }
            }
            // the score sums on the same arrays: the block count of loss_blocks(n, 0, ea), every thread of every block
            {
                const int sb = loss_blocks(v.n, 0, v.ea);
                const float *pr = predict + v.np, *pm = perim + v.np;
                double s[3] = {0, 0, 0};
                bool edge_bad = false;
                for (int bl = 0; bl < sb; ++bl)
                    for (int t = 0; t < kLossThreads; ++t)
                        score_accumulate(v.n, v.ea, pr, area + v.np * lda, lda, pm, adj + 2 * v.ap, len + v.ap * ldl, ldl,
                                         (int64_t)bl * kLossThreads + t, (int64_t)sb * kLossThreads, s[0], s[1], s[2], edge_bad);
                if (edge_bad != (bad_edge[k] == 1)) { printf("trial %d layout %d: score edge report %d\n", trial, k, edge_bad); return 1; }
                score_edges_skipped += edge_bad;
                if (!edge_bad) {
                    double w[3] = {0, 0, 0};
                    for (int64_t i = 0; i < v.n; ++i) {
                        w[0] += (double)(pr[i] * area[(v.np + i) * lda]);
                        if (pr[i] == 1.0f) w[2] += (double)pm[i];
                    }
                    for (int64_t e = 0; e < v.ea; ++e)
                        w[1] += (double)(pr[adj[2 * v.ap + e]] * pr[adj[2 * v.ap + v.ea + e]] * len[(v.ap + e) * ldl]);
                    for (int c = 0; c < 3; ++c)
                        if (fabs(s[c] - w[c]) > 1e-9 * (1.0 + fabs(w[c]))) { printf("trial %d layout %d score sum %d: %g vs %g\n", trial, k, c, s[c], w[c]); return 1; }
                }
            }
            ++layouts_walked;
        }
        free(area); free(len); free(adj); free(col); free(predict); free(perim);
        for (float *p : probs) free(p);
    }
    printf("ok: %ld layouts walked, %ld rejected for their offsets or counts, %ld maps and %ld score walks with a reported edge end\n",
           layouts_walked, rejected, edges_skipped, score_edges_skipped);
    return 0;
}
