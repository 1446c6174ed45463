// index_pq.cpp — IndexPQ (faiss/IndexPQ.cpp over faiss/IndexFlatCodes.cpp): a
// flat array of product-quantizer codes searched exhaustively.  The host keeps
// the reference's fields (pq, codes); HBM keeps the codes packed at a stride of
// roundup(code_size, 4) bytes and the codebooks, and a search is
// kern::pq_flat_search (kernels_pq_flat.hip) on them.
#include <cstring>

#include "../../include/faiss_amd.h"
#include "kernels.h"

namespace faiss_amd {

IndexPQStats indexPQ_stats;

namespace {
struct DevGuard {
    int prev = 0;
    explicit DevGuard(int dev) {
        ensure_hip();
        HIP_CHECK(hipGetDevice(&prev));
        if (prev != dev) HIP_CHECK(hipSetDevice(dev));
    }
    ~DevGuard() {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != prev) (void)hipSetDevice(prev);
    }
};

// before ProductQuantizer sizes its 2^nbits centroids
size_t checked_nbits(size_t nbits) {
    FAISS_THROW_IF_NOT_FMT(nbits >= 4 && nbits <= 8,
                           "IndexPQ: nbits = %zu is not supported on this path "
                           "(nbits 4, 5, 6, 7 and 8 are)",
                           nbits);
    return nbits;
}

const char* search_type_name(int t) {
    static const char* names[] = {"ST_PQ",  "ST_HE",         "ST_generalized_HE",
                                  "ST_SDC", "ST_polysemous", "ST_polysemous_generalize"};
    return t >= 0 && t < 6 ? names[t] : "unknown";
}
}  // namespace

IndexPQ::IndexPQ(int d_, size_t M, size_t nbits, MetricType metric)
        : Index(d_, metric), pq((size_t)d_, M, checked_nbits(nbits)) {
    FAISS_AMD_REQUIRE_BASIC_METRIC(metric, "IndexPQ");
    code_size = (M * nbits + 7) / 8;
    is_trained = false;
}

IndexPQ::IndexPQ() { is_trained = false; }

void IndexPQ::train(idx_t n, const float* x) {
    // faiss/IndexPQ.cpp:54-72 without polysemous training (not served)
    FAISS_THROW_IF_NOT_MSG(!do_polysemous_training,
                           "IndexPQ: polysemous training is not supported on this path");
    // faiss/impl/ProductQuantizer.cpp: at most 256 training points per centroid
    pq.train((size_t)std::min<idx_t>(n, (idx_t)pq.ksub * 256), x, device);
    is_trained = true;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexPQ::add(idx_t n, const float* x) {
    FAISS_THROW_IF_NOT(is_trained);
    if (n <= 0) return;
    const size_t old = codes.size();
    codes.resize(old + (size_t)n * code_size);
    pq.compute_codes(x, codes.data() + old, (size_t)n, device);
    ntotal += n;
    version_++;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexPQ::set_content(const float* centroids, idx_t n, const uint8_t* new_codes) {
    if (centroids) {
        memcpy(pq.centroids.data(), centroids, sizeof(float) * pq.centroids.size());
        is_trained = true;
    }
    if (new_codes) {
        FAISS_THROW_IF_NOT(n >= 0);
        codes.assign(new_codes, new_codes + (size_t)n * code_size);
        ntotal = n;
    }
    version_++;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexPQ::reset() {
    codes.clear();
    ntotal = 0;
    version_++;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexPQ::reconstruct(idx_t key, float* recons) const {
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    pq.decode(codes.data() + (size_t)key * code_size, recons);
}

void IndexPQ::reconstruct_n(idx_t i0, idx_t ni, float* recons) const {
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    for (idx_t i = 0; i < ni; i++)
        pq.decode(codes.data() + (size_t)(i0 + i) * code_size, recons + (size_t)i * d);
}

size_t IndexPQ::remove_ids(const IDSelector& sel) {
    idx_t j = 0;
    for (idx_t i = 0; i < ntotal; i++) {
        if (sel.is_member(i)) continue;
        if (i > j)
            memmove(codes.data() + (size_t)j * code_size, codes.data() + (size_t)i * code_size,
                    code_size);
        j++;
    }
    const size_t nremove = (size_t)(ntotal - j);
    if (nremove > 0) {
        ntotal = j;
        codes.resize((size_t)ntotal * code_size);
        version_++;
        std::lock_guard<std::recursive_mutex> g(mu_);
        dirty_ = true;
    }
    return nremove;
}

void IndexPQ::sync_device() const {
    std::lock_guard<std::recursive_mutex> g(mu_);
    if (!dirty_) return;
    FAISS_THROW_IF_NOT(codes.size() == (size_t)ntotal * code_size);
    FAISS_THROW_IF_NOT(pq.centroids.size() == pq.d * pq.ksub);
    DevGuard dg(device);
    hipStream_t s = stream();
    const size_t cs = (size_t)device_code_stride();
    d_pq_.reserve(sizeof(float) * pq.centroids.size());
    HIP_CHECK(hipMemcpyAsync(d_pq_.ptr, pq.centroids.data(), sizeof(float) * pq.centroids.size(),
                             hipMemcpyHostToDevice, s));
    d_codes_.reserve(std::max<size_t>((size_t)ntotal, 1) * cs);
    std::vector<uint8_t> padded;
    const uint8_t* src = codes.data();
    if (cs != code_size && ntotal > 0) {  // PQ5x5: 4-byte rows of 25-bit codes
        padded.assign((size_t)ntotal * cs, 0);
        for (idx_t i = 0; i < ntotal; i++)
            memcpy(padded.data() + (size_t)i * cs, codes.data() + (size_t)i * code_size, code_size);
        src = padded.data();
    }
    if (ntotal > 0)
        HIP_CHECK(hipMemcpyAsync(d_codes_.ptr, src, (size_t)ntotal * cs, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dirty_ = false;
    version_++;
}

void IndexPQ::check_search(const SearchParameters* params) const {
    int st = (int)search_type;
    if (params) {
        FAISS_THROW_IF_NOT_MSG(!params->sel, "selector not supported");
        if (auto p = dynamic_cast<const SearchParametersPQ*>(params)) st = p->search_type;
    }
    FAISS_THROW_IF_NOT_FMT(st == (int)ST_PQ,
                           "IndexPQ: search type %s is not supported on this path (ST_PQ is)",
                           search_type_name(st));
}

void IndexPQ::search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels,
                     const SearchParameters* params) const {
    check_search(params);
    Index::search(n, x, k, distances, labels, params);
    indexPQ_stats.nq += (size_t)n;
    indexPQ_stats.ncode += (size_t)n * (size_t)ntotal;
}

void IndexPQ::search_device(idx_t n, const float* x, int ldx, idx_t k, float* distances,
                            idx_t* labels, const SearchParameters* params,
                            hipStream_t stream) const {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT(k > 0);
    check_search(params);
    if (n <= 0) return;
    std::lock_guard<std::recursive_mutex> g(mu_);
    sync_device();
    DevGuard dg(device);
    kern::PQFlatArgs a;
    a.x = x;
    a.ldx = ldx;
    a.d = d;
    a.n = n;
    a.pq_cent = d_pq_.as<float>();
    a.M = (int)pq.M;
    a.dsub = (int)pq.dsub;
    a.nbits = (int)pq.nbits;
    a.codes = d_codes_.as<uint8_t>();
    a.cs = device_code_stride();
    a.ntotal = ntotal;
    a.k = (int)k;
    a.l2 = metric_type == METRIC_L2 ? 1 : 0;
    FAISS_THROW_IF_NOT_FMT(k <= kern::kMaxKExact, "k = %lld must be <= %d", (long long)k,
                           kern::kMaxKExact);
    order_.enter(stream);
    kern::pq_flat_search(a, s_part_, s_tab_, s_dense_, distances, labels, stream);
    order_.leave(stream);
}

}  // namespace faiss_amd
