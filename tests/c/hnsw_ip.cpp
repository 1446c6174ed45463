// faiss::IndexHNSWFlat(d, M, faiss::METRIC_INNER_PRODUCT) through the C++
// drop-in headers (include/faiss/), as a program written for the reference
// would use it: one add, hnsw.efSearch, search.
//
//   hnsw_ip_cpp <d> <M> <nb> <xb.f32> <nq> <xq.f32> <efSearch> <k> <out.bin>
// out.bin: D float32[nq*k], I int64[nq*k].
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include <faiss/IndexHNSW.h>
#include <faiss/MetricType.h>

static std::vector<float> read_f32(const char* fn, size_t n) {
    std::vector<float> v(n);
    std::ifstream f(fn, std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float)))) {
        fprintf(stderr, "short read: %s\n", fn);
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int d = atoi(argv[1]), M = atoi(argv[2]);
    const size_t nb = (size_t)atoll(argv[3]), nq = (size_t)atoll(argv[5]);
    const size_t k = (size_t)atoll(argv[8]);
    const std::vector<float> xb = read_f32(argv[4], nb * d), xq = read_f32(argv[6], nq * d);
    try {
        faiss::IndexHNSWFlat index(d, M, faiss::METRIC_INNER_PRODUCT);
        if (index.metric_type != faiss::METRIC_INNER_PRODUCT) return 3;
        index.add((faiss::idx_t)nb, xb.data());
        index.hnsw.efSearch = atoi(argv[7]);
        std::vector<float> D(nq * k);
        std::vector<faiss::idx_t> I(nq * k);
        index.search((faiss::idx_t)nq, xq.data(), (faiss::idx_t)k, D.data(), I.data());
        std::ofstream o(argv[9], std::ios::binary);
        o.write(reinterpret_cast<const char*>(D.data()), (std::streamsize)(D.size() * sizeof(float)));
        o.write(reinterpret_cast<const char*>(I.data()),
                (std::streamsize)(I.size() * sizeof(faiss::idx_t)));
        if (!o) return 4;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
