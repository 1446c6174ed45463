// binary_driver.cpp — runs the reference's binary indexes for
// scripts/make_golden_binary.py (linked against the reference objects that
// `make -C oracle/ref full` compiles; single OpenMP thread).
//
//   binary_driver flat d nb xb.bin out.faiss
//   binary_driver ivf  d nb xb.bin ids.bin nlist cent.bin out.faiss
//       (quantizer.add(centroids), is_trained = true, add_with_ids)
//   binary_driver search in.faiss nq xq.bin k use_heap nprobe max_codes D.bin I.bin
#include <faiss/IndexBinaryFlat.h>
#include <faiss/IndexBinaryIVF.h>
#include <faiss/index_io.h>
#include <omp.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

template <class T>
static std::vector<T> load(const char* fn, size_t n) {
    std::vector<T> v(n);
    FILE* f = fopen(fn, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "cannot read %zu items from %s\n", n, fn);
        exit(2);
    }
    fclose(f);
    return v;
}
template <class T>
static void save(const char* fn, const std::vector<T>& v) {
    FILE* f = fopen(fn, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
}

int main(int argc, char** argv) {
    omp_set_num_threads(1);
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "flat" && argc == 6) {
        const int d = atoi(argv[2]);
        const size_t nb = atol(argv[3]);
        faiss::IndexBinaryFlat ix(d);
        ix.add(nb, load<uint8_t>(argv[4], nb * d / 8).data());
        faiss::write_index_binary(&ix, argv[5]);
    } else if (mode == "ivf" && argc == 9) {
        const int d = atoi(argv[2]);
        const size_t nb = atol(argv[3]), nlist = atol(argv[6]);
        faiss::IndexBinaryFlat q(d);
        q.add(nlist, load<uint8_t>(argv[7], nlist * d / 8).data());
        faiss::IndexBinaryIVF ix(&q, d, nlist);
        ix.is_trained = true;
        ix.add_with_ids(nb, load<uint8_t>(argv[4], nb * d / 8).data(),
                        load<faiss::idx_t>(argv[5], nb).data());
        faiss::write_index_binary(&ix, argv[8]);
    } else if (mode == "search" && argc == 11) {
        std::unique_ptr<faiss::IndexBinary> ix(faiss::read_index_binary(argv[2]));
        const size_t nq = atol(argv[3]), k = atol(argv[5]);
        const bool use_heap = atoi(argv[6]) != 0;
        if (auto f = dynamic_cast<faiss::IndexBinaryFlat*>(ix.get())) f->use_heap = use_heap;
        if (auto v = dynamic_cast<faiss::IndexBinaryIVF*>(ix.get())) {
            v->use_heap = use_heap;
            v->nprobe = atol(argv[7]);
            v->max_codes = atol(argv[8]);
        }
        std::vector<int32_t> D(nq * k);
        std::vector<faiss::idx_t> I(nq * k);
        ix->search(nq, load<uint8_t>(argv[4], nq * ix->d / 8).data(), k, D.data(), I.data());
        save(argv[9], D);
        save(argv[10], I);
    } else {
        fprintf(stderr, "usage: see the head of scripts/binary_driver.cpp\n");
        return 2;
    }
    return 0;
}
