// index_sq.cpp — IndexScalarQuantizer (faiss/IndexScalarQuantizer.cpp:24-90 over
// faiss/IndexFlatCodes.cpp): a flat array of scalar-quantizer codes searched
// exhaustively.  The host keeps the reference's fields (sq, codes); HBM keeps
// the codes at their own pitch of code_size bytes and the trained ranges, and a
// search is kern::sq_flat_search (kernels_sq_flat.hip) on them.
#include <cstring>

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
}  // namespace

IndexScalarQuantizer::IndexScalarQuantizer(int d_, ScalarQuantizer::QuantizerType qtype,
                                           MetricType metric)
        : Index(d_, metric), sq((size_t)d_, qtype) {
    FAISS_AMD_REQUIRE_BASIC_METRIC(metric, "IndexScalarQuantizer");
    code_size = sq.code_size;
    // faiss/IndexScalarQuantizer.cpp:31-33: fp16 has nothing to train
    is_trained = qtype == ScalarQuantizer::QT_fp16;
}

IndexScalarQuantizer::IndexScalarQuantizer() { is_trained = false; }

void IndexScalarQuantizer::train(idx_t n, const float* x) {
    sq.train((size_t)n, x);
    is_trained = true;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexScalarQuantizer::add(idx_t n, const float* x) {
    FAISS_THROW_IF_NOT(is_trained);
    if (n <= 0) return;
    const size_t old = codes.size();
    codes.resize(old + (size_t)n * code_size);
    sq.compute_codes(x, codes.data() + old, (size_t)n);
    ntotal += n;
    version_++;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexScalarQuantizer::set_content(const float* trained, size_t nt, idx_t n,
                                       const uint8_t* new_codes) {
    if (trained) {
        const size_t want = sq.qtype == ScalarQuantizer::QT_8bit ? 2 * (size_t)d : 0;
        FAISS_THROW_IF_NOT_FMT(nt == want, "IndexScalarQuantizer: %zu trained values, expected %zu",
                               nt, want);
        sq.trained.assign(trained, trained + nt);
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

void IndexScalarQuantizer::reset() {
    codes.clear();
    ntotal = 0;
    version_++;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexScalarQuantizer::reconstruct(idx_t key, float* recons) const {
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    sq.decode(codes.data() + (size_t)key * code_size, recons, 1);
}

void IndexScalarQuantizer::reconstruct_n(idx_t i0, idx_t ni, float* recons) const {
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    if (ni > 0) sq.decode(codes.data() + (size_t)i0 * code_size, recons, (size_t)ni);
}

size_t IndexScalarQuantizer::remove_ids(const IDSelector& sel) {
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

void IndexScalarQuantizer::range_search(idx_t, const float*, float, RangeSearchResult*,
                                        const SearchParameters*) const {
    FAISS_THROW_MSG("IndexScalarQuantizer: range search not implemented");
}

void IndexScalarQuantizer::sync_device() const {
    std::lock_guard<std::recursive_mutex> g(mu_);
    if (!dirty_) return;
    ScalarQuantizer::check_supported((int)sq.qtype, (size_t)d);
    FAISS_THROW_IF_NOT(code_size == sq.code_size && codes.size() == (size_t)ntotal * code_size);
    FAISS_THROW_IF_NOT_MSG(sq.qtype != ScalarQuantizer::QT_8bit || !is_trained ||
                                   sq.trained.size() == 2 * (size_t)d,
                           "IndexScalarQuantizer: trained ranges missing");
    DevGuard dg(device);
    hipStream_t s = stream();
    d_trained_.reserve(sizeof(float) * std::max<size_t>(sq.trained.size(), 1));
    if (!sq.trained.empty())
        HIP_CHECK(hipMemcpyAsync(d_trained_.ptr, sq.trained.data(),
                                 sizeof(float) * sq.trained.size(), hipMemcpyHostToDevice, s));
    d_codes_.reserve(std::max<size_t>(codes.size(), 1));
    if (!codes.empty())
        HIP_CHECK(hipMemcpyAsync(d_codes_.ptr, codes.data(), codes.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dirty_ = false;
    version_++;
}

void IndexScalarQuantizer::search_device(idx_t n, const float* x, int ldx, idx_t k,
                                         float* distances, idx_t* labels,
                                         const SearchParameters* params,
                                         hipStream_t stream) const {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT_FMT(k <= kern::kMaxKExact, "k = %lld must be <= %d", (long long)k,
                           kern::kMaxKExact);
    if (n <= 0) return;
    std::lock_guard<std::recursive_mutex> g(mu_);
    sync_device();
    DevGuard dg(device);
    kern::SQFlatArgs a;
    a.x = x;
    a.ldx = ldx;
    a.d = d;
    a.n = n;
    a.qtype = (int)sq.qtype;
    a.trained = d_trained_.as<float>();
    a.codes = d_codes_.as<uint8_t>();
    a.ntotal = ntotal;
    a.k = (int)k;
    a.l2 = metric_type == METRIC_L2 ? 1 : 0;
    order_.enter(stream);
    try {
        if (params && params->sel && ntotal > 0) {
            // faiss/impl/ScalarQuantizer.cpp:2200-2203 (use_sel == 2): is_member(row)
            if (rowids_n_ != ntotal) {
                std::vector<idx_t> iota((size_t)ntotal);
                for (idx_t i = 0; i < ntotal; i++) iota[(size_t)i] = i;
                s_rowids_.reserve(sizeof(idx_t) * (size_t)ntotal);
                HIP_CHECK(hipMemcpyAsync(s_rowids_.ptr, iota.data(), sizeof(idx_t) * (size_t)ntotal,
                                         hipMemcpyHostToDevice, stream));
                HIP_CHECK(hipStreamSynchronize(stream));  // (iota is a host temporary)
                rowids_n_ = ntotal;
            }
            s_mask_.reserve((size_t)ntotal);
            params->sel->mark_device(s_rowids_.as<idx_t>(), ntotal, s_mask_.as<uint8_t>(), stream);
            a.mask = s_mask_.as<uint8_t>();
        }
        kern::sq_flat_search(a, s_dense_, s_sel_, distances, labels, stream, &ktimes);
    } catch (...) {
        order_.leave(stream);
        throw;
    }
    order_.leave(stream);
}

}  // namespace faiss_amd
