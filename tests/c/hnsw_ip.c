/* An inner-product IndexHNSWFlat through the C boundary (include/faiss_amd_c.h):
 * built with faiss_amd_IndexHNSWFlat_new_with (how = "new") or
 * faiss_index_factory (how = "factory"), filled in one add, searched.
 *
 *   hnsw_ip_c <how> <d> <M> <nb> <xb.f32> <nq> <xq.f32> <efSearch> <k> <out.bin>
 * out.bin: D float32[nq*k], I int64[nq*k]. */
#include <stdio.h>
#include <stdlib.h>

#include "faiss_amd_c.h"

static float* read_f32(const char* fn, size_t n) {
    float* v = (float*)malloc(n * sizeof(float));
    FILE* f = fopen(fn, "rb");
    if (!v || !f || fread(v, sizeof(float), n, f) != n) {
        fprintf(stderr, "short read: %s\n", fn);
        exit(2);
    }
    fclose(f);
    return v;
}

#define OK(call)                                                         \
    do {                                                                 \
        if ((call) != 0) {                                               \
            fprintf(stderr, "%s: %s\n", #call, faiss_get_last_error()); \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 11) return 2;
    const int factory = argv[1][0] == 'f';
    const int d = atoi(argv[2]), M = atoi(argv[3]);
    const size_t nb = (size_t)atoll(argv[4]), nq = (size_t)atoll(argv[6]);
    const int ef = atoi(argv[8]);
    const size_t k = (size_t)atoll(argv[9]);
    float* xb = read_f32(argv[5], nb * (size_t)d);
    float* xq = read_f32(argv[7], nq * (size_t)d);
    FaissIndex* ix = NULL;
    if (factory) {
        char desc[64];
        snprintf(desc, sizeof(desc), "HNSW%d,Flat", M);
        OK(faiss_index_factory(&ix, d, desc, METRIC_INNER_PRODUCT));
    } else {
        FaissIndexHNSW* h = NULL;
        OK(faiss_amd_IndexHNSWFlat_new_with(&h, d, M, METRIC_INNER_PRODUCT));
        ix = (FaissIndex*)h;
    }
    if (faiss_Index_metric_type(ix) != METRIC_INNER_PRODUCT) return 3;
    OK(faiss_Index_add(ix, (idx_t)nb, xb));
    faiss_amd_IndexHNSW_set_efSearch((FaissIndexHNSW*)ix, ef);
    float* D = (float*)malloc(nq * k * sizeof(float));
    idx_t* I = (idx_t*)malloc(nq * k * sizeof(idx_t));
    OK(faiss_Index_search(ix, (idx_t)nq, xq, (idx_t)k, D, I));
    FILE* o = fopen(argv[10], "wb");
    if (!o || fwrite(D, sizeof(float), nq * k, o) != nq * k ||
        fwrite(I, sizeof(idx_t), nq * k, o) != nq * k)
        return 4;
    fclose(o);
    faiss_Index_free(ix);
    free(D);
    free(I);
    free(xb);
    free(xq);
    return 0;
}
