// Stand-alone run of tilingnn_amd/csrc/greedy_rule.h -- the acceptance rule the single-layout and the K-layout greedy kernels
// share -- on the host.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/greedy_rule_test.cpp
// (tests/test_greedy_rule_host.py writes the cases, builds and runs this, and compares with tests/greedy_restatement.py).
//
// usage: greedy_rule_test <cases> <results>.  <cases>: int64 count, then per case int64 [8] = kind, n_sub, n_orig, has_inverse,
// ec, round (kinds 0, 2) or first_round (kind 1), max_rounds, has_prob; uint64 seed; inverse int64 [n_sub] if has_inverse;
// col int64 [2][ec]; prob float [n_sub] if has_prob; saved double [n_orig], alive int32 [n_orig], selected int32 [n_orig].
//   kind 0  one round with the header's functions alone, in the kernels' order: mean, beaten over the edges, accept, label
//   kind 1  the finishing block's phases with the header's flag constants (byte flags; nodes that have left are kept and skipped)
//   kind 2  saved[i] = greedy_uniform(seed, round, inverse[i])
// <results>: per case saved, alive, selected as they are afterwards, then int64 [4] = accepted, err, rounds run, nodes left.
// Every array is an exact-size heap block, so an index the rule should have refused is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "greedy_rule.h"

using namespace tgnn;

template <class T>
static std::vector<T> read_array(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}
template <class T>
static void write_array(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
}

struct Case {
    int64_t n_sub, ec;
    bool has_inverse;
    std::vector<int64_t> inverse, col;
    std::vector<float> prob;
    uint64_t seed;
    std::vector<double> saved;
    std::vector<int32_t> alive, selected;
    int64_t accepted = 0, err = 0, rounds_run = 0, left = 0;
    int64_t original(int64_t i) const { return has_inverse ? inverse[(size_t)i] : i; }
    bool inside(int64_t u, int64_t v) const { return u >= 0 && u < n_sub && v >= 0 && v < n_sub; }
};

static void round_walk(Case &c, int round) {
    std::vector<double> p((size_t)c.n_sub);
    std::vector<int> flags((size_t)c.n_sub);
    for (int64_t i = 0; i < c.n_sub; ++i) {                      // mean
        const int64_t o = c.original(i);
        p[i] = c.saved[o] = greedy_mean(c.saved[o], c.prob.empty() ? 1.0 : (double)c.prob[i], round);
        flags[i] = 0;
    }
    for (int64_t e = 0; e < c.ec; ++e) {                         // beaten
        const int64_t u = c.col[e], v = c.col[c.ec + e];
        if (!c.inside(u, v)) { c.err = 1; continue; }
        if (u == v) continue;
        flags[greedy_beaten_end(u, v, p[u], p[v])] = kGreedyBeaten;
    }
    for (int64_t i = 0; i < c.n_sub; ++i) {                      // accept
        if (flags[i] & kGreedyBeaten) continue;
        const int64_t o = c.original(i);
        if (greedy_accepts(p[i], c.seed, round, o)) {
            flags[i] = kGreedyAccepted;
            c.alive[o] = 0;
            c.selected[o] = round;
            ++c.accepted;
        }
    }
    for (int64_t e = 0; e < c.ec; ++e) {                         // label
        const int64_t u = c.col[e], v = c.col[c.ec + e];
        if (c.inside(u, v) && (flags[u] & kGreedyAccepted)) c.alive[c.original(v)] = 0;
    }
}

static void finish_walk(Case &c, int first_round, int max_rounds) {
    if (c.n_sub > kFinMaxNodes) exit(2);
    std::vector<double> p((size_t)c.n_sub);
    std::vector<unsigned char> flags((size_t)c.n_sub);
    for (int64_t i = 0; i < c.n_sub; ++i) flags[i] = c.alive[c.original(i)] ? 0 : kGreedyGone;
    for (int round = first_round;; ++round) {
        c.left = 0;
        for (int64_t i = 0; i < c.n_sub; ++i) {
            if (flags[i] & kGreedyGone) continue;
            ++c.left;
            const int64_t o = c.original(i);
            p[i] = c.saved[o] = greedy_mean(c.saved[o], 1.0, round);
            flags[i] = 0;
        }
        if (c.left == 0 || c.rounds_run >= max_rounds) break;
        ++c.rounds_run;
        for (int64_t e = 0; e < c.ec; ++e) {
            const int64_t u = c.col[e], v = c.col[c.ec + e];
            if (!c.inside(u, v)) { c.err = 1; continue; }
            if (u == v || ((flags[u] | flags[v]) & kGreedyGone)) continue;
            flags[greedy_beaten_end(u, v, p[u], p[v])] |= kGreedyBeaten;
        }
        for (int64_t i = 0; i < c.n_sub; ++i) {
            if (flags[i] & (kGreedyBeaten | kGreedyGone)) continue;
            const int64_t o = c.original(i);
            if (greedy_accepts(p[i], c.seed, round, o)) {
                flags[i] |= kGreedyAccepted;
                c.alive[o] = 0;
                c.selected[o] = round;
                ++c.accepted;
            }
        }
        for (int64_t e = 0; e < c.ec; ++e) {
            const int64_t u = c.col[e], v = c.col[c.ec + e];
            if (!c.inside(u, v)) continue;
            if ((flags[u] & kGreedyAccepted) && !(flags[v] & kGreedyGone)) {
                c.alive[c.original(v)] = 0;
                flags[v] |= kGreedyLeaving;
            }
        }
        for (int64_t i = 0; i < c.n_sub; ++i)
            if (flags[i] & (kGreedyAccepted | kGreedyLeaving)) flags[i] = kGreedyGone;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!f || !out) return 2;
    const int64_t n_cases = read_array<int64_t>(f, 1)[0];
    for (int64_t q = 0; q < n_cases; ++q) {
        const std::vector<int64_t> h = read_array<int64_t>(f, 8);
        Case c;
        c.n_sub = h[1];
        c.has_inverse = h[3] != 0;
        c.ec = h[4];
        c.seed = read_array<uint64_t>(f, 1)[0];
        c.inverse = read_array<int64_t>(f, c.has_inverse ? (size_t)c.n_sub : 0);
        c.col = read_array<int64_t>(f, 2 * (size_t)c.ec);
        c.prob = read_array<float>(f, h[7] ? (size_t)c.n_sub : 0);
        c.saved = read_array<double>(f, (size_t)h[2]);
        c.alive = read_array<int32_t>(f, (size_t)h[2]);
        c.selected = read_array<int32_t>(f, (size_t)h[2]);
        if (h[0] == 0) round_walk(c, (int)h[5]);
        else if (h[0] == 1) finish_walk(c, (int)h[5], (int)h[6]);
        else
            for (int64_t i = 0; i < c.n_sub; ++i) c.saved[i] = greedy_uniform(c.seed, (unsigned)h[5], (unsigned long long)c.inverse[i]);
        write_array(out, c.saved);
        write_array(out, c.alive);
        write_array(out, c.selected);
        write_array(out, std::vector<int64_t>{c.accepted, c.err, c.rounds_run, c.left});
    }
    fclose(f);
    if (fclose(out) != 0) return 2;
    printf("cases %lld\n", (long long)n_cases);
    return 0;
}
