// index_binary.cpp — IndexBinary, IndexBinaryFlat and IndexBinaryIVF
// (faiss/IndexBinary.cpp, IndexBinaryFlat.cpp, IndexBinaryIVF.cpp).  The host
// keeps the reference's fields (xb; invlists, direct_map, quantizer); HBM keeps
// the rows zero-padded to whole dwords — the flat array, or the lists back to
// back in one arena with int64 list offsets — and the searches are
// kernels_binary.hip's.
#include <cstring>
#include <numeric>

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

// n rows of cs bytes -> rows of W dwords, zero padded
std::vector<uint32_t> pad_rows(const uint8_t* x, size_t n, size_t cs, size_t W) {
    std::vector<uint32_t> out(std::max<size_t>(n * W, 1), 0u);
    if (cs == 4 * W) {
        if (n) memcpy(out.data(), x, n * cs);
    } else {
        for (size_t i = 0; i < n; i++) memcpy(out.data() + i * W, x + i * cs, cs);
    }
    return out;
}

void check_dims(idx_t d) {
    const bool d_ok = d >= 0 && d <= kern::BIN_MAX_D && (d & 7) == 0;
    FAISS_THROW_IF_NOT_FMT(d_ok, "IndexBinary: d = %lld bits must be a multiple of 8, at most %d",
                           (long long)d, kern::BIN_MAX_D);
}
}  // namespace

// ---------------------------------------------------------------- IndexBinary
IndexBinary::IndexBinary(idx_t d_) : d((int)d_), code_size((int)(d_ / 8)) { check_dims(d_); }
IndexBinary::~IndexBinary() = default;
void IndexBinary::train(idx_t, const uint8_t*) {}
void IndexBinary::add_with_ids(idx_t, const uint8_t*, const idx_t*) {
    FAISS_THROW_MSG("add_with_ids not implemented for this type of index");
}
void IndexBinary::range_search(idx_t, const uint8_t*, int, RangeSearchResult*,
                               const SearchParameters*) const {
    FAISS_THROW_MSG(std::string(class_name()) + ": range_search is not supported on this path");
}
size_t IndexBinary::remove_ids(const IDSelector&) {
    FAISS_THROW_MSG("remove_ids not implemented for this type of index");
}
void IndexBinary::reconstruct(idx_t, uint8_t*) const {
    FAISS_THROW_MSG("reconstruct not implemented for this type of index");
}
void IndexBinary::reconstruct_n(idx_t i0, idx_t ni, uint8_t* recons) const {
    for (idx_t i = 0; i < ni; i++) reconstruct(i0 + i, recons + (size_t)i * code_size);
}
hipStream_t IndexBinary::stream() const { return device_context(device).stream; }

// host entry: pad the queries to dwords, upload, search_device, download
void IndexBinary::search(idx_t n, const uint8_t* x, idx_t k, int32_t* distances, idx_t* labels,
                         const SearchParameters* params) const {
    FAISS_THROW_IF_NOT(k > 0);
    if (n <= 0) return;
    DevGuard g(device);
    sync_device();
    hipStream_t s = stream();
    const size_t W = (size_t)device_words();
    std::lock_guard<std::mutex> hg(host_mu_);
    const std::vector<uint32_t> xp = pad_rows(x, (size_t)n, (size_t)code_size, W);
    h_x_.reserve(4 * (size_t)n * W);
    h_d_.reserve(sizeof(int32_t) * n * k);
    h_i_.reserve(sizeof(idx_t) * n * k);
    HIP_CHECK(hipMemcpyAsync(h_x_.ptr, xp.data(), 4 * (size_t)n * W, hipMemcpyHostToDevice, s));
    search_device(n, h_x_.as<uint32_t>(), k, h_d_.as<int32_t>(), h_i_.as<idx_t>(), params, s);
    HIP_CHECK(hipMemcpyAsync(distances, h_d_.ptr, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipMemcpyAsync(labels, h_i_.ptr, sizeof(idx_t) * n * k, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------- IndexBinaryFlat
IndexBinaryFlat::IndexBinaryFlat(idx_t d_) : IndexBinary(d_) {}

void IndexBinaryFlat::add(idx_t n, const uint8_t* x) {
    FAISS_THROW_IF_NOT(n >= 0);
    xb.insert(xb.end(), x, x + (size_t)n * code_size);
    ntotal += n;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexBinaryFlat::reset() {
    xb.clear();
    ntotal = 0;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

size_t IndexBinaryFlat::remove_ids(const IDSelector& sel) {
    idx_t j = 0;
    for (idx_t i = 0; i < ntotal; i++) {
        if (sel.is_member(i)) continue;
        if (i > j)
            memmove(xb.data() + (size_t)j * code_size, xb.data() + (size_t)i * code_size,
                    code_size);
        j++;
    }
    const size_t nremove = (size_t)(ntotal - j);
    if (nremove > 0) {
        ntotal = j;
        xb.resize((size_t)ntotal * code_size);
        std::lock_guard<std::recursive_mutex> g(mu_);
        dirty_ = true;
    }
    return nremove;
}

void IndexBinaryFlat::reconstruct(idx_t key, uint8_t* recons) const {
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    memcpy(recons, xb.data() + (size_t)key * code_size, code_size);
}

void IndexBinaryFlat::sync_device() const {
    std::lock_guard<std::recursive_mutex> g(mu_);
    if (!dirty_) return;
    FAISS_THROW_IF_NOT(xb.size() == (size_t)ntotal * code_size);
    DevGuard dg(device);
    hipStream_t s = stream();
    const size_t W = (size_t)device_words();
    const std::vector<uint32_t> rows = pad_rows(xb.data(), (size_t)ntotal, (size_t)code_size, W);
    d_codes_.reserve(4 * rows.size());
    HIP_CHECK(hipMemcpyAsync(d_codes_.ptr, rows.data(), 4 * rows.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dirty_ = false;
}

void IndexBinaryFlat::search(idx_t n, const uint8_t* x, idx_t k, int32_t* distances,
                             idx_t* labels, const SearchParameters* params) const {
    FAISS_THROW_IF_NOT_MSG(!params, "search params not supported for this index");
    IndexBinary::search(n, x, k, distances, labels, params);
}

void IndexBinaryFlat::search_device(idx_t n, const uint32_t* x, idx_t k, int32_t* distances,
                                    idx_t* labels, const SearchParameters* params,
                                    hipStream_t stream) const {
    FAISS_THROW_IF_NOT_MSG(!params, "search params not supported for this index");
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT_FMT(k <= kern::kMaxKExact, "k = %lld must be <= %d", (long long)k,
                           kern::kMaxKExact);
    if (n <= 0) return;
    std::lock_guard<std::recursive_mutex> g(mu_);
    sync_device();
    DevGuard dg(device);
    order_.enter(stream);
    kern::binary_flat_search(x, n, d, d_codes_.as<uint32_t>(), ntotal, (int)k, s_scan_, distances,
                             labels, stream);
    order_.leave(stream);
}

// ---------------------------------------------------------------- IndexBinaryIVF
IndexBinaryIVF::IndexBinaryIVF(IndexBinary* q, size_t d_, size_t nlist_)
        : IndexBinary((idx_t)d_),
          invlists(new ArrayInvertedLists(nlist_, d_ / 8)),
          quantizer(q),
          nlist(nlist_) {
    FAISS_THROW_IF_NOT(q && (size_t)q->d == d_);
    check_quantizer();
    is_trained = q->is_trained && (size_t)q->ntotal == nlist;
}
IndexBinaryIVF::IndexBinaryIVF() = default;
IndexBinaryIVF::~IndexBinaryIVF() {
    if (own_fields) delete quantizer;
}

void IndexBinaryIVF::check_quantizer() const {
    FAISS_THROW_IF_NOT_MSG(dynamic_cast<const IndexBinaryFlat*>(quantizer),
                           "IndexBinaryIVF: only an IndexBinaryFlat quantizer is supported "
                           "(IndexBinaryHNSW, IndexBinaryHash and IndexBinaryFromFloat are not)");
}

void IndexBinaryIVF::train(idx_t n, const uint8_t* x) {
    check_quantizer();
    if (!(quantizer->is_trained && (size_t)quantizer->ntotal == nlist)) {
        FAISS_THROW_IF_NOT_FMT((size_t)n >= nlist, "%lld training vectors for %zu centroids",
                               (long long)n, nlist);
        // faiss/Clustering.cpp:85-115: at most 256 points per centroid, a random
        // subset (seeded) when there are more
        const idx_t nt = std::min<idx_t>(n, (idx_t)nlist * 256);
        std::vector<idx_t> pick((size_t)n);
        std::iota(pick.begin(), pick.end(), (idx_t)0);
        if (nt < n) {
            std::mt19937_64 rng(1234);
            for (idx_t i = 0; i < nt; i++)
                std::swap(pick[(size_t)i], pick[(size_t)(i + (idx_t)(rng() % (uint64_t)(n - i)))]);
        }
        std::vector<float> xf((size_t)nt * d);
        for (idx_t i = 0; i < nt; i++) {
            const uint8_t* row = x + (size_t)pick[(size_t)i] * code_size;
            for (int j = 0; j < d; j++)
                xf[(size_t)i * d + j] = ((row[j >> 3] >> (j & 7)) & 1) ? 1.f : -1.f;
        }
        std::vector<float> cent(nlist * (size_t)d);
        kmeans_train(d, nt, xf.data(), (int)nlist, niter, 1234, cent.data(), device, verbose);
        std::vector<uint8_t> cb(nlist * (size_t)code_size, 0);  // real_to_binary: bit = (v > 0)
        for (size_t i = 0; i < nlist; i++)
            for (int j = 0; j < d; j++)
                if (cent[i * d + j] > 0) cb[i * code_size + (j >> 3)] |= (uint8_t)(1u << (j & 7));
        quantizer->reset();
        quantizer->add((idx_t)nlist, cb.data());
        quantizer->is_trained = true;
    }
    is_trained = true;
}

void IndexBinaryIVF::add(idx_t n, const uint8_t* x) { add_with_ids(n, x, nullptr); }

void IndexBinaryIVF::add_with_ids(idx_t n, const uint8_t* x, const idx_t* xids) {
    FAISS_THROW_IF_NOT(is_trained);
    if (n <= 0) return;
    direct_map.check_can_add(xids);
    std::vector<int32_t> cd((size_t)n);
    std::vector<idx_t> ci((size_t)n);
    quantizer->search(n, x, 1, cd.data(), ci.data());
    for (idx_t i = 0; i < n; i++) {
        const idx_t id = xids ? xids[i] : ntotal + i;
        const idx_t l = ci[i];
        if (l < 0) {
            direct_map.add_single_id(id, -1, 0);
            continue;
        }
        const size_t off = invlists->list_size((size_t)l);
        invlists->add_entries((size_t)l, 1, &id, x + (size_t)i * code_size);
        direct_map.add_single_id(id, l, off);
    }
    ntotal += n;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexBinaryIVF::reset() {
    invlists->reset();
    direct_map.clear();
    ntotal = 0;
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
}

void IndexBinaryIVF::set_direct_map_type(DirectMap::Type type) {
    direct_map.set_type(type, invlists.get(), (size_t)ntotal);
}

void IndexBinaryIVF::reconstruct(idx_t key, uint8_t* recons) const {
    const idx_t lo = direct_map.get(key);
    memcpy(recons,
           invlists->get_codes((size_t)lo_listno(lo)) + (size_t)lo_offset(lo) * code_size,
           code_size);
}

void IndexBinaryIVF::reconstruct_n(idx_t i0, idx_t ni, uint8_t* recons) const {
    // faiss/IndexBinaryIVF.cpp:183-205: one pass over the lists, ids in range
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    for (size_t l = 0; l < nlist; l++) {
        const idx_t* ids = invlists->get_ids(l);
        const uint8_t* codes = invlists->get_codes(l);
        for (size_t o = 0; o < invlists->list_size(l); o++) {
            const idx_t id = ids[o];
            if (id < i0 || id >= i0 + ni) continue;
            memcpy(recons + (size_t)(id - i0) * code_size, codes + o * code_size, code_size);
        }
    }
}

void IndexBinaryIVF::merge_from(IndexBinaryIVF&, idx_t) {
    FAISS_THROW_MSG("IndexBinaryIVF: merge_from is not supported on this path");
}

void IndexBinaryIVF::sync_device() const {
    std::lock_guard<std::recursive_mutex> g(mu_);
    quantizer->sync_device();
    if (!dirty_) return;
    DevGuard dg(device);
    hipStream_t s = stream();
    const size_t W = (size_t)device_words(), cs = (size_t)code_size;
    std::vector<int64_t> off(nlist + 1, 0);
    std::vector<uint32_t> len(std::max<size_t>(nlist, 1), 0);
    max_list_len_ = 0;
    for (size_t l = 0; l < nlist; l++) {
        const size_t sz = invlists->list_size(l);
        FAISS_THROW_IF_NOT_MSG(sz < ((size_t)1 << 32), "IndexBinaryIVF: a list of 2^32 rows");
        len[l] = (uint32_t)sz;
        off[l + 1] = off[l] + (int64_t)sz;
        max_list_len_ = std::max(max_list_len_, len[l]);
    }
    const size_t rows = (size_t)off[nlist];
    std::vector<uint32_t> codes(std::max<size_t>(rows * W, 1), 0u);
    std::vector<int64_t> ids(std::max<size_t>(rows, 1), -1);
    for (size_t l = 0; l < nlist; l++) {
        const uint8_t* c = invlists->get_codes(l);
        for (size_t o = 0; o < len[l]; o++)
            memcpy(codes.data() + ((size_t)off[l] + o) * W, c + o * cs, cs);
        if (len[l]) memcpy(ids.data() + off[l], invlists->get_ids(l), sizeof(int64_t) * len[l]);
    }
    d_codes_.reserve(4 * codes.size());
    d_ids_.reserve(8 * ids.size());
    d_list_off_.reserve(8 * off.size());
    d_list_len_.reserve(4 * len.size());
    HIP_CHECK(hipMemcpyAsync(d_codes_.ptr, codes.data(), 4 * codes.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ids_.ptr, ids.data(), 8 * ids.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_list_off_.ptr, off.data(), 8 * off.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_list_len_.ptr, len.data(), 4 * len.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dirty_ = false;
}

namespace {
// nprobe / max_codes of the call; a selector is refused
void ivf_params(const IndexBinaryIVF* ix, const SearchParameters* params, size_t* nprobe,
                size_t* max_codes) {
    *nprobe = ix->nprobe;
    *max_codes = ix->max_codes;
    if (params) {
        FAISS_THROW_IF_NOT_MSG(!params->sel,
                               "IndexBinaryIVF: an IDSelector is not supported on this path");
        auto p = dynamic_cast<const SearchParametersIVF*>(params);
        FAISS_THROW_IF_NOT_MSG(p, "IndexBinaryIVF: params type invalid");
        *nprobe = p->nprobe;
        *max_codes = p->max_codes;
    }
    FAISS_THROW_IF_NOT_MSG(!ix->per_invlist_search,
                           "IndexBinaryIVF: per_invlist_search is not supported on this path");
    FAISS_THROW_IF_NOT(*nprobe > 0);
}
}  // namespace

void IndexBinaryIVF::scan_device(idx_t n, const uint32_t* x, idx_t k, const idx_t* coarse, int np,
                                 size_t max_codes_, int32_t* distances, idx_t* labels,
                                 hipStream_t s) const {
    s_assign_.reserve(sizeof(int32_t) * (size_t)n * np);
    kern::binary_probes(coarse, n, np, d_list_len_.as<uint32_t>(), (int)nlist, (int64_t)max_codes_,
                        s_assign_.as<int32_t>(), s);
    kern::binary_ivf_scan(x, n, d, d_codes_.as<uint32_t>(), d_ids_.as<int64_t>(),
                          d_list_off_.as<int64_t>(), d_list_len_.as<uint32_t>(), max_list_len_,
                          s_assign_.as<int32_t>(), np, (int)k, use_heap, s_scan_, distances, labels,
                          s);
}

void IndexBinaryIVF::search(idx_t n, const uint8_t* x, idx_t k, int32_t* distances, idx_t* labels,
                            const SearchParameters* params) const {
    size_t np, mc;
    ivf_params(this, params, &np, &mc);
    IndexBinary::search(n, x, k, distances, labels, params);
}

void IndexBinaryIVF::search_device(idx_t n, const uint32_t* x, idx_t k, int32_t* distances,
                                   idx_t* labels, const SearchParameters* params,
                                   hipStream_t stream) const {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT_FMT(k <= kern::kMaxKExact, "k = %lld must be <= %d", (long long)k,
                           kern::kMaxKExact);
    check_quantizer();
    size_t np_, mc;
    ivf_params(this, params, &np_, &mc);
    if (n <= 0) return;
    const int np = (int)std::min(nlist, np_);  // faiss/IndexBinaryIVF.cpp:122
    std::lock_guard<std::recursive_mutex> g(mu_);
    sync_device();
    DevGuard dg(device);
    order_.enter(stream);
    s_coarse_d_.reserve(sizeof(int32_t) * (size_t)n * np);
    s_coarse_i_.reserve(sizeof(idx_t) * (size_t)n * np);
    quantizer->search_device(n, x, np, s_coarse_d_.as<int32_t>(), s_coarse_i_.as<idx_t>(), nullptr,
                             stream);
    scan_device(n, x, k, s_coarse_i_.as<idx_t>(), np, mc, distances, labels, stream);
    order_.leave(stream);
}

void IndexBinaryIVF::search_preassigned(idx_t n, const uint8_t* x, idx_t k, const idx_t* assign,
                                        const int32_t*, int32_t* distances, idx_t* labels,
                                        bool store_pairs, const SearchParametersIVF* params) const {
    FAISS_THROW_IF_NOT_MSG(!store_pairs, "IndexBinaryIVF: store_pairs is not supported on this path");
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT_FMT(k <= kern::kMaxKExact, "k = %lld must be <= %d", (long long)k,
                           kern::kMaxKExact);
    size_t np_, mc;
    ivf_params(this, params, &np_, &mc);
    if (n <= 0) return;
    const int np = (int)std::min(nlist, np_);
    for (size_t i = 0; i < (size_t)n * np; i++)
        FAISS_THROW_IF_NOT_FMT(assign[i] < (idx_t)nlist, "Invalid key=%lld nlist=%zu",
                               (long long)assign[i], nlist);
    // host_mu_ before mu_, the order of IndexBinary::search
    std::lock_guard<std::mutex> hg(host_mu_);
    std::lock_guard<std::recursive_mutex> g(mu_);
    sync_device();
    DevGuard dg(device);
    hipStream_t s = stream();
    const size_t W = (size_t)device_words();
    const std::vector<uint32_t> xp = pad_rows(x, (size_t)n, (size_t)code_size, W);
    h_x_.reserve(4 * (size_t)n * W);
    h_d_.reserve(sizeof(int32_t) * n * k);
    h_i_.reserve(sizeof(idx_t) * n * k);
    s_coarse_i_.reserve(sizeof(idx_t) * (size_t)n * np);
    order_.enter(s);
    HIP_CHECK(hipMemcpyAsync(h_x_.ptr, xp.data(), 4 * (size_t)n * W, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(s_coarse_i_.ptr, assign, sizeof(idx_t) * (size_t)n * np,
                             hipMemcpyHostToDevice, s));
    scan_device(n, h_x_.as<uint32_t>(), k, s_coarse_i_.as<idx_t>(), np, mc, h_d_.as<int32_t>(),
                h_i_.as<idx_t>(), s);
    order_.leave(s);
    HIP_CHECK(hipMemcpyAsync(distances, h_d_.ptr, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipMemcpyAsync(labels, h_i_.ptr, sizeof(idx_t) * n * k, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace faiss_amd
