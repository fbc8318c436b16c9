// The unit functions of csrc/batch_union.hip (`__host__ __device__`) run on the HOST under AddressSanitizer: 3 000 random packed
// sets and id lists (empty members, repeats, odd edge counts), exact-size heap buffers, units past the end of every array,
// wide loads / stores on and off; every output element against the definition of the union.  No GPU is used.
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -x hip \
//         scratch/batch_union_host_check.cpp -o build/batch_union_host_check && build/batch_union_host_check
#include "../tilingnn_amd/csrc/batch_union.hip"
#include <vector>
#include <random>
#include <cstdio>
#include <cstdlib>
#include <cstring>
namespace tgnn { void set_error(const char *, ...) {} }
int main() {
    std::mt19937_64 rng(1);
    long checked = 0;
    for (int trial = 0; trial < 3000; ++trial) {
        int K = 1 + rng() % 6, fx = 1 + rng() % 5, fe = 1 + rng() % 6;
        std::vector<int64_t> np(K + 1, 0), ap(K + 1, 0), cp(K + 1, 0);
        for (int k = 0; k < K; ++k) {
            np[k + 1] = np[k] + (rng() % 4 == 0 ? 0 : rng() % 13);
            ap[k + 1] = ap[k] + (rng() % 4 == 0 ? 0 : rng() % 17);
            cp[k + 1] = cp[k] + (rng() % 4 == 0 ? 0 : rng() % 9);
        }
        // exact-size heap buffers, 16-byte aligned by aligned_alloc through posix_memalign
        auto alloc = [](size_t bytes) { void *p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 1)) abort(); return p; };
        float *x = (float *)alloc(np[K] * fx * 4), *attr = (float *)alloc(ap[K] * fe * 4);
        int64_t *adj = (int64_t *)alloc(ap[K] * 16), *col = (int64_t *)alloc(cp[K] * 16);
        for (int64_t i = 0; i < np[K] * fx; ++i) x[i] = (float)(rng() % 100000);
        for (int64_t i = 0; i < ap[K] * fe; ++i) attr[i] = (float)(rng() % 100000);
        for (int64_t i = 0; i < 2 * ap[K]; ++i) adj[i] = rng() % 1000;
        for (int64_t i = 0; i < 2 * cp[K]; ++i) col[i] = rng() % 1000;
        int B = 1 + rng() % 7;
        std::vector<int64_t> tab(4 * B + 3);
        int64_t *ids = tab.data(), *no = ids + B, *ao = ids + 2 * B + 1, *co = ids + 3 * B + 2;
        no[0] = ao[0] = co[0] = 0;
        for (int b = 0; b < B; ++b) {
            ids[b] = rng() % K;
            no[b + 1] = no[b] + np[ids[b] + 1] - np[ids[b]];
            ao[b + 1] = ao[b] + ap[ids[b] + 1] - ap[ids[b]];
            co[b + 1] = co[b] + cp[ids[b] + 1] - cp[ids[b]];
        }
        int64_t N = no[B], EA = ao[B], EC = co[B];
        float *xo = (float *)alloc(N * fx * 4), *ato = (float *)alloc(EA * fe * 4);
        int64_t *ado = (int64_t *)alloc(EA * 16), *clo = (int64_t *)alloc(EC * 16);
        memset(xo, 0xff, N * fx * 4); memset(ato, 0xff, EA * fe * 4); memset(ado, 0xff, EA * 16); memset(clo, 0xff, EC * 16);
        bool wide_ld = trial % 3 != 0, wide_st = trial % 2 != 0;
        int64_t ux = (N * fx + 3) / 4, ua = (EA * fe + 3) / 4;
        for (int64_t u = 0; u < ux + 2; ++u) tgnn::copy_rows_unit(x, xo, np.data(), ids, no, B, fx, wide_ld, wide_st, u);
        for (int64_t u = 0; u < ua + 2; ++u) tgnn::copy_rows_unit(attr, ato, ap.data(), ids, ao, B, fe, wide_ld, wide_st, u);
        for (int64_t u = 0; u < EA + 2; ++u) tgnn::copy_index_unit(adj, ado, ap.data(), ids, ao, no, B, wide_ld, wide_st, u);
        for (int64_t u = 0; u < EC + 2; ++u) tgnn::copy_index_unit(col, clo, cp.data(), ids, co, no, B, wide_ld, wide_st, u);
        for (int b = 0; b < B; ++b) {
            int64_t k = ids[b];
            for (int64_t r = 0; r < np[k + 1] - np[k]; ++r) for (int c = 0; c < fx; ++c, ++checked)
                if (xo[(no[b] + r) * fx + c] != x[(np[k] + r) * fx + c]) { printf("x mismatch trial %d\n", trial); return 1; }
            int64_t ek = ap[k + 1] - ap[k];
            for (int64_t e = 0; e < ek; ++e) {
                for (int c = 0; c < fe; ++c, ++checked)
                    if (ato[(ao[b] + e) * fe + c] != attr[(ap[k] + e) * fe + c]) { printf("attr mismatch trial %d\n", trial); return 1; }
                for (int r = 0; r < 2; ++r, ++checked)
                    if (ado[r * EA + ao[b] + e] != adj[2 * ap[k] + r * ek + e] + no[b]) { printf("adj mismatch trial %d\n", trial); return 1; }
            }
            int64_t ck = cp[k + 1] - cp[k];
            for (int64_t e = 0; e < ck; ++e) for (int r = 0; r < 2; ++r, ++checked)
                if (clo[r * EC + co[b] + e] != col[2 * cp[k] + r * ck + e] + no[b]) { printf("col mismatch trial %d\n", trial); return 1; }
        }
        free(x); free(attr); free(adj); free(col); free(xo); free(ato); free(ado); free(clo);
    }
    printf("ok, %ld elements checked\n", checked);
    return 0;
}
