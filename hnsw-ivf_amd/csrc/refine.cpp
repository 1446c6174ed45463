// refine.cpp — IndexRefine / IndexRefineFlat (faiss/IndexRefine.cpp).
//
// The wrapper searches k_base = idx_t(k * k_factor) candidates in its base
// index, replaces their distances by the flat storage's exact ones
// (kernels_refine.hip, the reference's fp32 order) and keeps the k the
// reference's reorder_2_heaps keeps (kernels_exact.hip k_ex_select: arrival
// rank = position in the base row).  Base search, distances and select are
// queued on the caller's stream with no host synchronisation in between.
#include "../../include/faiss_amd.h"
#include "kernels.h"

namespace faiss_amd {

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

const IndexRefineSearchParameters* refine_params(const SearchParameters* params_in) {
    if (!params_in) return nullptr;
    auto params = dynamic_cast<const IndexRefineSearchParameters*>(params_in);
    FAISS_THROW_IF_NOT_MSG(params, "IndexRefineFlat params have incorrect type");
    return params;
}
}  // namespace

// ---------------------------------------------------------------- IndexRefine
IndexRefine::IndexRefine(Index* base, Index* refine)
        : Index(base->d, base->metric_type), base_index(base), refine_index(refine) {
    // faiss/IndexRefine.cpp:21-34
    device = base->device;
    if (refine != nullptr) {
        FAISS_THROW_IF_NOT_FMT(dynamic_cast<const IndexFlat*>(refine),
                               "IndexRefine: a refine index of type %s is not served (IndexFlat only)",
                               index_type_name(refine));
        FAISS_THROW_IF_NOT(base->d == refine->d);
        FAISS_THROW_IF_NOT(base->metric_type == refine->metric_type);
        is_trained = base->is_trained && refine->is_trained;
        FAISS_THROW_IF_NOT(base->ntotal == refine->ntotal);
    }  // other case is useful only to construct an IndexRefineFlat
    ntotal = base->ntotal;
}

IndexRefine::IndexRefine() = default;

IndexRefine::~IndexRefine() {
    if (own_fields) delete base_index;
    if (own_refine_index) delete refine_index;
}

const IndexFlat* IndexRefine::flat_storage() const {
    FAISS_THROW_IF_NOT(refine_index);
    auto rf = dynamic_cast<const IndexFlat*>(refine_index);
    FAISS_THROW_IF_NOT_FMT(rf, "IndexRefine: a refine index of type %s is not served (IndexFlat only)",
                           index_type_name(refine_index));
    return rf;
}

void IndexRefine::train(idx_t n, const float* x) {
    base_index->train(n, x);
    refine_index->train(n, x);
    is_trained = true;
}

void IndexRefine::add(idx_t n, const float* x) {
    FAISS_THROW_IF_NOT(is_trained);
    base_index->add(n, x);
    refine_index->add(n, x);
    ntotal = refine_index->ntotal;
    version_++;
}

void IndexRefine::reset() {
    base_index->reset();
    refine_index->reset();
    ntotal = 0;
    version_++;
}

void IndexRefine::reconstruct(idx_t key, float* recons) const {
    refine_index->reconstruct(key, recons);
}

void IndexRefine::sync_device() const {
    if (base_index) base_index->sync_device();
    if (refine_index) refine_index->sync_device();
}

void IndexRefine::fold_device_stats() const {
    if (base_index) base_index->fold_device_stats();
}

void IndexRefine::search_device(idx_t n, const float* x, int ldx, idx_t k, float* distances,
                                idx_t* labels, const SearchParameters* params_in,
                                hipStream_t s) const {
    // faiss/IndexRefine.cpp:274-337
    const IndexRefineSearchParameters* params = refine_params(params_in);
    const idx_t k_base = params ? idx_t(k * params->k_factor) : idx_t(k * k_factor);
    const SearchParameters* base_params = params ? params->base_index_params : nullptr;
    FAISS_THROW_IF_NOT(k_base >= k);
    FAISS_THROW_IF_NOT(base_index);
    FAISS_THROW_IF_NOT(refine_index);
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT(is_trained);
    const IndexFlat* rf = flat_storage();
    if (n == 0) return;
    DevGuard dg(device);
    sync_device();
    const float* xb = rf->device_vectors();
    const bool l2 = metric_type == METRIC_L2;
    std::lock_guard<std::recursive_mutex> g(mu_);
    order_.enter(s);
    // leave() also when the base search throws (a k_base beyond its limit):
    // earlier chunks may have used the scratch on s
    struct Leave {
        StreamOrder& o;
        hipStream_t s;
        ~Leave() {
            try {
                o.leave(s);
            } catch (...) {
            }
        }
    } leave{order_, s};
    // queries per pass: at most 1 GiB of candidate scratch (distances, labels, keys)
    const idx_t qc = std::max<idx_t>(1, std::min<idx_t>(n, ((idx_t)1 << 30) / (16 * k_base)));
    const bool in_place = k_base == k;  // the base result is re-ordered where it lies
    if (!in_place) {
        s_bd_.reserve(sizeof(float) * qc * k_base);
        s_bi_.reserve(sizeof(idx_t) * qc * k_base);
    }
    s_keys_.reserve(sizeof(uint32_t) * qc * k_base);
    for (idx_t q0 = 0; q0 < n; q0 += qc) {
        const idx_t nq = std::min(qc, n - q0);
        float* bd = in_place ? distances + q0 * k : s_bd_.as<float>();
        idx_t* bi = in_place ? labels + q0 * k : s_bi_.as<idx_t>();
        // a k_base beyond the base index's own limit throws there
        base_index->search_device(nq, x + q0 * ldx, ldx, k_base, bd, bi, base_params, s);
        ScopedKernelTimer tm(&ktimes, "refine", 2.0 * nq * k_base * d, s);
        kern::refine_flat_distances(x + q0 * ldx, ldx, nq, d, l2, bi, k_base, xb, rf->ld(),
                                    rf->ntotal, s_keys_.as<uint32_t>(), s);
        kern::refine_select(s_keys_.as<uint32_t>(), bi, nq, k_base, (int)k, l2,
                            distances + q0 * k, labels + q0 * k, s, &s_sel_);
    }
}

void IndexRefine::range_search(idx_t n, const float* x, float radius, RangeSearchResult* result,
                               const SearchParameters* params_in) const {
    // faiss/IndexRefine.cpp:169-206
    const IndexRefineSearchParameters* params = refine_params(params_in);
    FAISS_THROW_IF_NOT(base_index);
    const IndexFlat* rf = flat_storage();
    base_index->range_search(n, x, radius, result, params ? params->base_index_params : nullptr);
    const size_t tot = result->lims.empty() ? 0 : result->lims[(size_t)n];
    if (n == 0 || tot == 0) return;
    DevGuard dg(device);
    rf->sync_device();
    hipStream_t s = stream();
    const int ldx = ld();
    static_assert(sizeof(size_t) == sizeof(unsigned long long), "lims are 64-bit");
    DeviceBuffer bx, bl, bi, bd;
    bx.reserve(sizeof(float) * n * ldx);
    bl.reserve(sizeof(size_t) * (n + 1));
    bi.reserve(sizeof(idx_t) * tot);
    bd.reserve(sizeof(float) * tot);
    if (ldx != d) HIP_CHECK(hipMemsetAsync(bx.ptr, 0, sizeof(float) * n * ldx, s));
    HIP_CHECK(hipMemcpy2DAsync(bx.ptr, sizeof(float) * ldx, x, sizeof(float) * d,
                               sizeof(float) * d, n, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(bl.ptr, result->lims.data(), sizeof(size_t) * (n + 1),
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(bi.ptr, result->labels.data(), sizeof(idx_t) * tot,
                             hipMemcpyHostToDevice, s));
    kern::refine_range_distances(bx.as<float>(), ldx, n, d, metric_type == METRIC_L2,
                                 bl.as<unsigned long long>(), bi.as<idx_t>(),
                                 rf->device_vectors(), rf->ld(), rf->ntotal, bd.as<float>(), s);
    HIP_CHECK(hipMemcpyAsync(result->distances.data(), bd.ptr, sizeof(float) * tot,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------- IndexRefineFlat
namespace {
// the wrapper's flat storage, on the base index's device
std::unique_ptr<IndexFlat> new_storage(const Index* base) {
    auto flat = std::make_unique<IndexFlat>(base->d, base->metric_type);
    flat->device = base->device;
    return flat;
}
}  // namespace

IndexRefineFlat::IndexRefineFlat(Index* base) : IndexRefine(base, nullptr) {
    // faiss/IndexRefine.cpp:251-260.  The storage is held here until every
    // check has passed, so a throw leaves nothing behind.
    auto flat = new_storage(base);
    FAISS_THROW_IF_NOT(base->ntotal == flat->ntotal);  // IndexRefine(base, refine)'s check
    FAISS_THROW_IF_NOT_MSG(base->ntotal == 0, "base_index should be empty in the beginning");
    is_trained = base->is_trained;
    refine_index = flat.release();
    own_refine_index = true;
}

IndexRefineFlat::IndexRefineFlat(Index* base, const float* xb) : IndexRefine(base, nullptr) {
    // faiss/IndexRefine.cpp:262-268
    auto flat = new_storage(base);
    flat->add(base->ntotal, xb);
    is_trained = base->is_trained;
    refine_index = flat.release();
    own_refine_index = true;
}

IndexRefineFlat::IndexRefineFlat() : IndexRefine() { own_refine_index = true; }

}  // namespace faiss_amd
