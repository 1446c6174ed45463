// Fixture driver for scripts/make_golden_mutation.py: runs the reference CPU
// library's IndexIVF::remove_ids / update_vectors / reconstruct family and
// direct maps, and records what they leave.  Test infrastructure only;
// compiled against the reference's public headers and the objects
// `make -C oracle/ref full` leaves under oracle/_ref/fobj, into oracle/_ref/
// (never committed, never linked into the product).
//
//   mutation_driver index <factory> <l2|ip> <d> <nb> <xb.f32> <nq> <xq.f32> <base.faiss>
//                   <out.rec> [<array.faiss> <hash.faiss>]
//   mutation_driver sqtable <out.rec>
//
// index: builds (train + add of xb, sequential ids), writes base.faiss (no
// direct map) and the records below; every mutation starts from a fresh
// read_index(base.faiss).  With the two extra names it also writes the index
// with an Array map and with a Hashtable map.
// sqtable: ScalarQuantizer(8, QT_8bit)::decode of all 256 codes against 8
// (vmin, vdiff) pairs.
//
// out.rec: records [u32 len][name][u8 type 0 f32 / 1 i64 / 2 u8 / 3 u32]
// [u32 ndim][u64 dims][data].  Names (S = range | batch | array | hash):
//   rm_S_sel (the ids / bounds), rm_S_count, rm_S_sizes [nlist], rm_S_ids,
//   rm_S_codes (lists concatenated), rm_S_k{1,10,100}_{D,I}
//   hash_map [n][2] (id, entry; ascending id) after the Hashtable removal
//   array_refusal (the exception text of remove_ids under an Array map)
//   upd_ids, upd_x, upd_{array,hash}_{sizes,ids,codes,map}
//   rec_keys, rec_x (reconstruct through an Array map)
//   recn_range (i0, ni), recn_x (reconstruct_n after the range removal over
//   rows prefilled with the word 0x7fc0dead)
//   sar_{D,I,R} (search_and_reconstruct, 16 queries, k 5, nprobe 4; R as u32)
//   pad_xq, pad_k, pad_{D,I,R} (nprobe 1, k beyond the probed list)
#include <omp.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <faiss/IndexIVF.h>
#include <faiss/impl/FaissException.h>
#include <faiss/impl/IDSelector.h>
#include <faiss/impl/ScalarQuantizer.h>
#include <faiss/index_factory.h>
#include <faiss/index_io.h>
#include <faiss/invlists/DirectMap.h>

namespace {

using faiss::idx_t;

std::vector<float> read_f32(const std::string& fn, size_t n) {
    std::vector<float> v(n);
    std::ifstream f(fn, std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float))))
        throw std::runtime_error("short read: " + fn);
    return v;
}

struct Rec {
    FILE* f;
    void put(const std::string& name, int type, const std::vector<uint64_t>& dims,
             const void* data, size_t bytes) {
        const uint32_t len = (uint32_t)name.size(), nd = (uint32_t)dims.size();
        const uint8_t t = (uint8_t)type;
        fwrite(&len, 4, 1, f);
        fwrite(name.data(), 1, len, f);
        fwrite(&t, 1, 1, f);
        fwrite(&nd, 4, 1, f);
        fwrite(dims.data(), 8, nd, f);
        if (bytes) fwrite(data, 1, bytes, f);
    }
    void f32(const std::string& n, const std::vector<float>& v, std::vector<uint64_t> dims) {
        put(n, 0, dims, v.data(), v.size() * 4);
    }
    void u32(const std::string& n, const std::vector<float>& v, std::vector<uint64_t> dims) {
        put(n, 3, dims, v.data(), v.size() * 4);
    }
    void i64(const std::string& n, const std::vector<idx_t>& v, std::vector<uint64_t> dims) {
        put(n, 1, dims, v.data(), v.size() * 8);
    }
    void i64(const std::string& n, const std::vector<idx_t>& v) { i64(n, v, {v.size()}); }
    void u8(const std::string& n, const std::vector<uint8_t>& v) {
        put(n, 2, {v.size()}, v.data(), v.size());
    }
    void str(const std::string& n, const std::string& s) {
        put(n, 2, {s.size()}, s.data(), s.size());
    }
};

faiss::IndexIVF* load(const std::string& fn) {
    auto* ivf = dynamic_cast<faiss::IndexIVF*>(faiss::read_index(fn.c_str()));
    if (!ivf) throw std::runtime_error("not an IndexIVF: " + fn);
    ivf->nprobe = 4;
    return ivf;
}

void dump_lists(Rec& r, const std::string& p, const faiss::IndexIVF* ivf) {
    std::vector<idx_t> sizes, ids;
    std::vector<uint8_t> codes;
    for (size_t l = 0; l < ivf->nlist; l++) {
        const size_t n = ivf->invlists->list_size(l);
        sizes.push_back((idx_t)n);
        faiss::InvertedLists::ScopedIds si(ivf->invlists, l);
        faiss::InvertedLists::ScopedCodes sc(ivf->invlists, l);
        ids.insert(ids.end(), si.get(), si.get() + n);
        codes.insert(codes.end(), sc.get(), sc.get() + n * ivf->code_size);
    }
    r.i64(p + "_sizes", sizes);
    r.i64(p + "_ids", ids);
    r.u8(p + "_codes", codes);
}

void dump_map(Rec& r, const std::string& name, const faiss::IndexIVF* ivf) {
    std::vector<idx_t> v;
    if (ivf->direct_map.type == faiss::DirectMap::Array) {
        for (size_t i = 0; i < ivf->direct_map.array.size(); i++) {
            v.push_back((idx_t)i);
            v.push_back(ivf->direct_map.array[i]);
        }
    } else {
        std::vector<std::pair<idx_t, idx_t>> p(ivf->direct_map.hashtable.begin(),
                                               ivf->direct_map.hashtable.end());
        std::sort(p.begin(), p.end());
        for (auto& e : p) {
            v.push_back(e.first);
            v.push_back(e.second);
        }
    }
    r.i64(name, v, {v.size() / 2, 2});
}

void dump_search(Rec& r, const std::string& p, const faiss::IndexIVF* ivf, size_t nq,
                 const float* xq) {
    for (idx_t k : {1, 10, 100}) {
        std::vector<idx_t> assign(nq * ivf->nprobe), I(nq * k);
        std::vector<float> cd(nq * ivf->nprobe), D(nq * k);
        ivf->quantizer->search(nq, xq, ivf->nprobe, cd.data(), assign.data());
        ivf->search_preassigned(nq, xq, k, assign.data(), cd.data(), D.data(), I.data(), false);
        r.f32(p + "_k" + std::to_string(k) + "_D", D, {nq, (uint64_t)k});
        r.i64(p + "_k" + std::to_string(k) + "_I", I, {nq, (uint64_t)k});
    }
}

int run_index(int argc, char** argv) {
    const std::string factory = argv[2], metric = argv[3];
    const int d = atoi(argv[4]);
    const size_t nb = (size_t)atol(argv[5]);
    const std::string xbf = argv[6];
    const size_t nq = (size_t)atol(argv[7]);
    const std::string xqf = argv[8], base = argv[9], out = argv[10];
    const auto xb = read_f32(xbf, nb * d), xq = read_f32(xqf, nq * d);
    {
        std::unique_ptr<faiss::Index> ix(faiss::index_factory(
                d, factory.c_str(),
                metric == "ip" ? faiss::METRIC_INNER_PRODUCT : faiss::METRIC_L2));
        ix->train(nb, xb.data());
        ix->add(nb, xb.data());
        faiss::write_index(ix.get(), base.c_str());
    }
    FILE* f = fopen(out.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + out);
    Rec r{f};
    const idx_t N = (idx_t)nb;

    // ---- removal without a map
    std::vector<idx_t> batch_ids, array_ids, hash_ids;
    for (idx_t i = 3; i < N; i += 7) batch_ids.push_back(i);
    for (idx_t i = 0; i < 150; i++) array_ids.push_back(N - 1 - i);
    for (idx_t i = 0; i < 100; i++) array_ids.push_back(5 * i + 1);
    for (idx_t i = 50; i < 350; i++) hash_ids.push_back(i);
    hash_ids.push_back(60);      // a repeat
    hash_ids.push_back(N + 3000);  // absent
    for (idx_t i = N - 100; i < N - 50; i++) hash_ids.push_back(i);
    const std::vector<idx_t> range_ids = {100, 400};
    {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        dump_lists(r, "base", ivf.get());
        dump_search(r, "base", ivf.get(), nq, xq.data());
    }
    for (const std::string s : {"range", "batch", "array"}) {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        size_t nrm;
        if (s == "range") {
            faiss::IDSelectorRange sel(range_ids[0], range_ids[1]);
            nrm = ivf->remove_ids(sel);
            r.i64("rm_range_sel", range_ids);
        } else if (s == "batch") {
            faiss::IDSelectorBatch sel(batch_ids.size(), batch_ids.data());
            nrm = ivf->remove_ids(sel);
            r.i64("rm_batch_sel", batch_ids);
        } else {
            faiss::IDSelectorArray sel(array_ids.size(), array_ids.data());
            nrm = ivf->remove_ids(sel);
            r.i64("rm_array_sel", array_ids);
        }
        r.i64("rm_" + s + "_count", {(idx_t)nrm, ivf->ntotal});
        dump_lists(r, "rm_" + s, ivf.get());
        dump_search(r, "rm_" + s, ivf.get(), nq, xq.data());
        if (s == "range") {
            const idx_t i0 = 50, ni = 150;  // 50 stored ids, then 100 removed ones
            std::vector<float> x((size_t)ni * d);
            const uint32_t w = 0x7fc0deadu;
            for (auto& v : x) memcpy(&v, &w, 4);
            ivf->reconstruct_n(i0, ni, x.data());
            r.i64("recn_range", {i0, ni});
            r.u32("recn_x", x, {(uint64_t)ni, (uint64_t)d});
        }
    }
    // ---- removal through a map
    {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        ivf->set_direct_map_type(faiss::DirectMap::Hashtable);
        faiss::IDSelectorArray sel(hash_ids.size(), hash_ids.data());
        const size_t nrm = ivf->remove_ids(sel);
        r.i64("rm_hash_sel", hash_ids);
        r.i64("rm_hash_count", {(idx_t)nrm, ivf->ntotal});
        dump_lists(r, "rm_hash", ivf.get());
        dump_search(r, "rm_hash", ivf.get(), nq, xq.data());
        dump_map(r, "hash_map", ivf.get());
        // any other selector is refused
        try {
            faiss::IDSelectorRange rs(0, 10);
            ivf->remove_ids(rs);
            r.str("hash_refusal", "");
        } catch (const faiss::FaissException& e) {
            r.str("hash_refusal", e.msg);
        }
    }
    {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        ivf->make_direct_map(true);
        try {
            faiss::IDSelectorRange rs(0, 10);
            ivf->remove_ids(rs);
            r.str("array_refusal", "");
        } catch (const faiss::FaissException& e) {
            r.str("array_refusal", e.msg);
        }
        // reconstruct through the map
        std::vector<idx_t> keys = {0, 1, 7, N / 2, N - 200, N - 1, 199, N - 1 - 199};
        std::vector<float> x(keys.size() * d);
        for (size_t i = 0; i < keys.size(); i++) ivf->reconstruct(keys[i], x.data() + i * d);
        r.i64("rec_keys", keys);
        r.u32("rec_x", x, {keys.size(), (uint64_t)d});
        if (argc > 12) faiss::write_index(ivf.get(), argv[11]);
    }
    if (argc > 12) {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        ivf->set_direct_map_type(faiss::DirectMap::Hashtable);
        faiss::write_index(ivf.get(), argv[12]);
    }
    // ---- update_vectors
    {
        std::vector<idx_t> uids = {5, 17, N - 1, 300, 301, 302, 0, N / 2, 1234 % N, 77,
                                   78, N - 200, 199, 640, 641, 9};
        std::vector<float> ux(xq.begin(), xq.begin() + uids.size() * d);
        r.i64("upd_ids", uids);
        r.f32("upd_x", ux, {uids.size(), (uint64_t)d});
        for (const std::string s : {"array", "hash"}) {
            std::unique_ptr<faiss::IndexIVF> ivf(load(base));
            ivf->set_direct_map_type(s == "array" ? faiss::DirectMap::Array
                                                  : faiss::DirectMap::Hashtable);
            ivf->update_vectors((int)uids.size(), uids.data(), ux.data());
            dump_lists(r, "upd_" + s, ivf.get());
            dump_map(r, "upd_" + s + "_map", ivf.get());
            dump_search(r, "upd_" + s, ivf.get(), nq, xq.data());
        }
    }
    // ---- search_and_reconstruct
    {
        std::unique_ptr<faiss::IndexIVF> ivf(load(base));
        const size_t n = 16, k = 5;
        std::vector<float> D(n * k), R(n * k * d);
        std::vector<idx_t> I(n * k);
        ivf->search_and_reconstruct(n, xq.data(), k, D.data(), I.data(), R.data());
        r.f32("sar_D", D, {n, k});
        r.i64("sar_I", I, {n, k});
        r.u32("sar_R", R, {n, k, (uint64_t)d});
        // nprobe 1, k beyond the probed list: the two shortest non-empty
        // lists' centroids as queries
        std::vector<std::pair<size_t, size_t>> ls;
        for (size_t l = 0; l < ivf->nlist; l++)
            if (ivf->invlists->list_size(l)) ls.push_back({ivf->invlists->list_size(l), l});
        std::sort(ls.begin(), ls.end());
        std::vector<float> pq(2 * d);
        for (int i = 0; i < 2; i++) ivf->quantizer->reconstruct(ls[i].second, pq.data() + i * d);
        const size_t pk = ls[1].first + 5;
        ivf->nprobe = 1;
        std::vector<float> PD(2 * pk), PR(2 * pk * d);
        std::vector<idx_t> PI(2 * pk);
        ivf->search_and_reconstruct(2, pq.data(), pk, PD.data(), PI.data(), PR.data());
        r.f32("pad_xq", pq, {2, (uint64_t)d});
        r.i64("pad_k", {(idx_t)pk});
        r.f32("pad_D", PD, {2, pk});
        r.i64("pad_I", PI, {2, pk});
        r.u32("pad_R", PR, {2, pk, (uint64_t)d});
    }
    fclose(f);
    return 0;
}

int run_sqtable(char** argv) {
    FILE* f = fopen(argv[2], "wb");
    if (!f) throw std::runtime_error("cannot write out");
    Rec r{f};
    const int d = 8;
    faiss::ScalarQuantizer sq(d, faiss::ScalarQuantizer::QT_8bit);
    const std::vector<float> vmin = {0.f, -1.f, 0.1f, -3.7f, 1e-3f, 12345.678f, -0.333333f, 2.5f};
    const std::vector<float> vdiff = {1.f, 2.f, 0.7f, 9.1f, 3e-3f, 0.001f, 0.666667f, 1e6f};
    sq.trained = vmin;
    sq.trained.insert(sq.trained.end(), vdiff.begin(), vdiff.end());
    std::vector<uint8_t> codes(256 * d);
    for (int c = 0; c < 256; c++)
        for (int j = 0; j < d; j++) codes[c * d + j] = (uint8_t)c;
    std::vector<float> x(256 * d);
    sq.decode(codes.data(), x.data(), 256);
    r.f32("sq_vmin", vmin, {8});
    r.f32("sq_vdiff", vdiff, {8});
    r.u32("sq_decode", x, {256, 8});
    fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    omp_set_num_threads(1);
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "index" && argc >= 11) return run_index(argc, argv);
        if (mode == "sqtable" && argc >= 3) return run_sqtable(argv);
        fprintf(stderr, "usage: see the head of scripts/mutation_driver.cpp\n");
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "mutation_driver: %s\n", e.what());
        return 1;
    }
}
