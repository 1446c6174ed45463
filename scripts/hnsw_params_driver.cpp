// Fixture driver for scripts/make_golden_hnsw_params.py: runs the reference
// CPU library's HNSW searches with SearchParametersHNSW / SearchParametersIVF,
// index-level flags and IDSelectors, and records D, I and faiss::hnsw_stats.
// Test infrastructure only; compiled against the reference's public headers
// and the objects `make -C oracle/ref full` leaves under oracle/_ref/fobj, into
// oracle/_ref/ (never committed, never linked into the product).
//
//   hnsw_params_driver build <factory> <d> <nb> <xb.f32> <out.faiss> [l2|ip]
//   hnsw_params_driver run <index.faiss> <d> <nq> <xq.f32> <jobs.txt> <outdir>
//   hnsw_params_driver coarse <index.faiss> <d> <nq> <xq.f32> <efSearch> <k> <out.bin>
//
// build: the metric defaults to l2; an index that needs training (IVF) is
// trained on xb before the add.  coarse: the IndexIVF's quantizer (an
// IndexHNSW) searched on its own at efSearch; out.bin as a job's, without
// the stats.
//
// jobs.txt, one case per line:
//   name k how efSearch check bounded sel nprobe
// how: params  - a SearchParametersHNSW with the three values and sel
//      index   - the three values set on the index (the quantizer's for an
//                IVF index), params == nullptr
//      cleared - both flags cleared on the index, a default-constructed
//                SearchParametersHNSW passed (the values on the line are unused)
// sel: none | range:<imin>:<imax> | batch:<start>:<step>:<count> |
//      notbatch:<start>:<step>:<count>
// nprobe: 0 for an IndexHNSW; else the index is an IndexIVF whose quantizer
// is the IndexHNSW, and the HNSW parameters are its quantizer_params.
// <outdir>/<name>.bin: D float32[nq*k], I int64[nq*k], n1 n2 ndis nhops uint64.
#include <omp.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <faiss/IndexHNSW.h>
#include <faiss/IndexIVF.h>
#include <faiss/impl/HNSW.h>
#include <faiss/impl/IDSelector.h>
#include <faiss/index_factory.h>
#include <faiss/index_io.h>

namespace {

std::vector<float> read_f32(const std::string& fn, size_t n) {
    std::vector<float> v(n);
    std::ifstream f(fn, std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float))))
        throw std::runtime_error("short read: " + fn);
    return v;
}

struct Sel {
    std::unique_ptr<faiss::IDSelector> inner, outer;
    faiss::IDSelector* get() const { return outer ? outer.get() : inner.get(); }
};

Sel parse_sel(const std::string& spec) {
    Sel s;
    if (spec == "none") return s;
    std::vector<std::string> part;
    std::stringstream ss(spec);
    for (std::string t; std::getline(ss, t, ':');) part.push_back(t);
    if (part[0] == "range" && part.size() == 3) {
        s.inner.reset(new faiss::IDSelectorRange(std::stoll(part[1]), std::stoll(part[2])));
    } else if ((part[0] == "batch" || part[0] == "notbatch") && part.size() == 4) {
        std::vector<faiss::idx_t> ids;
        const long long start = std::stoll(part[1]), step = std::stoll(part[2]);
        for (long long i = 0; i < std::stoll(part[3]); i++) ids.push_back(start + i * step);
        s.inner.reset(new faiss::IDSelectorBatch(ids.size(), ids.data()));
        if (part[0] == "notbatch") s.outer.reset(new faiss::IDSelectorNot(s.inner.get()));
    } else {
        throw std::runtime_error("bad selector: " + spec);
    }
    return s;
}

int build(char** a) {
    const int d = atoi(a[1]);
    const size_t nb = (size_t)atoll(a[2]);
    const std::string metric = a[5] ? a[5] : "l2";
    if (metric != "l2" && metric != "ip") throw std::runtime_error("bad metric: " + metric);
    std::unique_ptr<faiss::Index> ix(faiss::index_factory(
            d, a[0], metric == "ip" ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2));
    const std::vector<float> xb = read_f32(a[3], nb * d);
    if (!ix->is_trained) ix->train((faiss::idx_t)nb, xb.data());
    ix->add((faiss::idx_t)nb, xb.data());
    faiss::write_index(ix.get(), a[4]);
    return 0;
}

int run(char** a) {
    std::unique_ptr<faiss::Index> ix(faiss::read_index(a[0]));
    const int d = atoi(a[1]);
    const size_t nq = (size_t)atoll(a[2]);
    const std::vector<float> xq = read_f32(a[3], nq * d);
    const std::string outdir = a[5];
    auto* ivf = dynamic_cast<faiss::IndexIVF*>(ix.get());
    auto* hx = dynamic_cast<faiss::IndexHNSW*>(ivf ? ivf->quantizer : ix.get());
    if (!hx) throw std::runtime_error("no IndexHNSW in the index");
    const faiss::HNSW saved = hx->hnsw;
    std::ifstream jobs(a[4]);
    std::string name, how, selspec;
    long long k, ef, check, bounded, nprobe;
    while (jobs >> name >> k >> how >> ef >> check >> bounded >> selspec >> nprobe) {
        if ((nprobe > 0) != (ivf != nullptr)) throw std::runtime_error("nprobe vs index: " + name);
        const Sel sel = parse_sel(selspec);
        faiss::SearchParametersHNSW hp;
        const faiss::SearchParameters* params = nullptr;
        hx->hnsw.efSearch = saved.efSearch;
        hx->hnsw.check_relative_distance = saved.check_relative_distance;
        hx->hnsw.search_bounded_queue = saved.search_bounded_queue;
        if (how == "params") {
            hp.efSearch = (int)ef;
            hp.check_relative_distance = check != 0;
            hp.bounded_queue = bounded != 0;
            hp.sel = sel.get();
            params = &hp;
        } else if (how == "index") {
            hx->hnsw.efSearch = (int)ef;
            hx->hnsw.check_relative_distance = check != 0;
            hx->hnsw.search_bounded_queue = bounded != 0;
        } else if (how == "cleared") {
            hx->hnsw.check_relative_distance = false;
            hx->hnsw.search_bounded_queue = false;
            params = &hp;
        } else {
            throw std::runtime_error("bad how: " + how);
        }
        faiss::SearchParametersIVF ip;
        if (ivf) {
            ivf->nprobe = (size_t)nprobe;
            if (params) {
                ip.nprobe = (size_t)nprobe;
                ip.quantizer_params = &hp;
                params = &ip;
            }
        }
        std::vector<float> D(nq * k);
        std::vector<faiss::idx_t> I(nq * k);
        faiss::hnsw_stats.reset();
        ix->search((faiss::idx_t)nq, xq.data(), k, D.data(), I.data(), params);
        const uint64_t st[4] = {faiss::hnsw_stats.n1, faiss::hnsw_stats.n2, faiss::hnsw_stats.ndis,
                                faiss::hnsw_stats.nhops};
        std::ofstream o(outdir + "/" + name + ".bin", std::ios::binary);
        o.write(reinterpret_cast<const char*>(D.data()), (std::streamsize)(D.size() * sizeof(float)));
        o.write(reinterpret_cast<const char*>(I.data()),
                (std::streamsize)(I.size() * sizeof(faiss::idx_t)));
        o.write(reinterpret_cast<const char*>(st), sizeof(st));
        if (!o) throw std::runtime_error("write failed: " + name);
    }
    return 0;
}

int coarse(char** a) {
    std::unique_ptr<faiss::Index> ix(faiss::read_index(a[0]));
    const int d = atoi(a[1]);
    const size_t nq = (size_t)atoll(a[2]);
    const std::vector<float> xq = read_f32(a[3], nq * d);
    auto* ivf = dynamic_cast<faiss::IndexIVF*>(ix.get());
    auto* hx = ivf ? dynamic_cast<faiss::IndexHNSW*>(ivf->quantizer) : nullptr;
    if (!hx) throw std::runtime_error("no IndexIVF over an IndexHNSW");
    hx->hnsw.efSearch = atoi(a[4]);
    const size_t k = (size_t)atoll(a[5]);
    std::vector<float> D(nq * k);
    std::vector<faiss::idx_t> I(nq * k);
    hx->search((faiss::idx_t)nq, xq.data(), (faiss::idx_t)k, D.data(), I.data());
    std::ofstream o(a[6], std::ios::binary);
    o.write(reinterpret_cast<const char*>(D.data()), (std::streamsize)(D.size() * sizeof(float)));
    o.write(reinterpret_cast<const char*>(I.data()),
            (std::streamsize)(I.size() * sizeof(faiss::idx_t)));
    if (!o) throw std::runtime_error("write failed");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    omp_set_num_threads(1);
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "build" && (argc == 7 || argc == 8)) return build(argv + 2);  // (argv[argc] is null)
        if (cmd == "coarse" && argc == 9) return coarse(argv + 2);
        if (cmd == "run" && argc == 8) return run(argv + 2);
        fprintf(stderr, "usage: see the head of hnsw_params_driver.cpp\n");
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "hnsw_params_driver: %s\n", e.what());
        return 1;
    }
}
