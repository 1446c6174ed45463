// pretransform.cpp — VectorTransform / LinearTransform and IndexPreTransform
// (faiss/VectorTransform.cpp, faiss/IndexPreTransform.cpp).
//
// A transform is applied by kern::linear_transform (kernels_transform.hip) on
// device rows; the host entry points upload, run the same kernel and
// download, so host and device callers get the same bits.  IndexPreTransform
// runs its chain between two scratch buffers of its own, the last transform
// writing the zero-padded query rows the sub-index's search_device reads, on
// the caller's stream with no host synchronisation.
#include <cmath>

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

int ld4(int d) { return (int)roundup((size_t)d, 4); }

// rows per pass of a host call: at most 256 MiB of device rows in and out
idx_t host_chunk(idx_t n, int ld_in, int ld_out) {
    const idx_t cap = ((idx_t)64 << 20) / std::max(1, ld_in + ld_out);
    return std::max<idx_t>(1, std::min(n, cap));
}

// device rows of ld floats into host rows of d, synchronous (one linear copy
// when the rows are not padded)
void download_rows(float* dst, int d, const float* src, int ld, idx_t n, hipStream_t s) {
    if (ld == d)
        HIP_CHECK(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)n * d, hipMemcpyDeviceToHost, s));
    else
        HIP_CHECK(hipMemcpy2DAsync(dst, sizeof(float) * d, src, sizeof(float) * ld,
                                   sizeof(float) * d, n, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// host rows [n][d_src] -> fn(device rows in, device rows out) -> host [n][d_dst]
template <class Fn>
void host_pass(idx_t n, const float* src, int d_src, float* dst, int d_dst, Fn&& fn) {
    if (n <= 0) return;
    DevGuard dg(current_device());
    hipStream_t s = device_context(current_device()).stream;
    const int ls = ld4(d_src), ldd = ld4(d_dst);
    const idx_t qc = host_chunk(n, ls, ldd);
    DeviceBuffer bi, bo;
    bi.reserve(sizeof(float) * qc * ls);
    bo.reserve(sizeof(float) * qc * ldd);
    for (idx_t q0 = 0; q0 < n; q0 += qc) {
        const idx_t nq = std::min(qc, n - q0);
        upload_rows(bi.as<float>(), ls, src + q0 * d_src, d_src, nq, s);
        fn(nq, bi.as<float>(), ls, bo.as<float>(), ldd, s);
        download_rows(dst + q0 * d_dst, d_dst, bo.as<float>(), ldd, nq, s);
    }
}
}  // namespace

// ---------------------------------------------------------------- VectorTransform
void VectorTransform::train(idx_t, const float*) {}  // faiss/VectorTransform.cpp:146

float* VectorTransform::apply(idx_t n, const float* x) const {
    std::unique_ptr<float[]> xt(new float[(size_t)n * d_out]);
    apply_noalloc(n, x, xt.get());
    return xt.release();
}

void VectorTransform::apply_noalloc(idx_t n, const float* x, float* xt) const {
    sync_device();
    host_pass(n, x, d_in, xt, d_out,
              [&](idx_t nq, const float* a, int lda, float* o, int ldo, hipStream_t s) {
                  apply_device(nq, a, lda, o, ldo, s);
              });
}

void VectorTransform::reverse_transform(idx_t n, const float* xt, float* x) const {
    sync_device();
    host_pass(n, xt, d_out, x, d_in,
              [&](idx_t nq, const float* a, int lda, float* o, int ldo, hipStream_t s) {
                  reverse_device(nq, a, lda, o, ldo, s);
              });
}

void VectorTransform::reverse_device(idx_t, const float*, int, float*, int, hipStream_t) const {
    FAISS_THROW_MSG("reverse transform not implemented");
}

// ---------------------------------------------------------------- LinearTransform
LinearTransform::LinearTransform(int d_in, int d_out, bool have_bias)
        : VectorTransform(d_in, d_out), have_bias(have_bias) {
    is_trained = false;  // will be trained when A and b are initialized
}

void LinearTransform::no_training(const char* what) const {
    FAISS_THROW_FMT("training %s is not served; read a trained transform or set A", what);
}

void LinearTransform::sync_device() const {
    FAISS_THROW_IF_NOT_MSG(is_trained, "Transformation not trained yet");
    FAISS_THROW_IF_NOT_FMT(d_in >= 1 && d_in <= kern::kTransformMaxDim && d_out >= 1 &&
                                   d_out <= kern::kTransformMaxDim,
                           "LinearTransform: d_in = %d / d_out = %d outside 1 .. %d", d_in, d_out,
                           kern::kTransformMaxDim);
    const size_t na = (size_t)d_out * d_in;
    FAISS_THROW_IF_NOT_MSG(A.size() >= na, "Transformation matrix not initialized");
    FAISS_THROW_IF_NOT_MSG(!have_bias || b.size() >= (size_t)d_out, "Bias not initialized");
    std::lock_guard<std::mutex> g(mu_);
    const size_t nb = have_bias ? (size_t)d_out : 0;
    int dev = 0;
    ensure_hip();
    HIP_CHECK(hipGetDevice(&dev));
    if (uploaded_ && d_A_.device == dev && up_A_.size() == na && up_b_.size() == nb &&
        memcmp(up_A_.data(), A.data(), sizeof(float) * na) == 0 &&
        (nb == 0 || memcmp(up_b_.data(), b.data(), sizeof(float) * nb) == 0))
        return;
    HIP_CHECK(hipDeviceSynchronize());  // queued kernels may still read the old matrix
    d_A_.reserve(sizeof(float) * na);
    d_b_.reserve(sizeof(float) * std::max<size_t>(nb, 1));
    up_A_.assign(A.begin(), A.begin() + na);
    up_b_.assign(b.begin(), b.begin() + nb);
    HIP_CHECK(hipMemcpy(d_A_.ptr, up_A_.data(), sizeof(float) * na, hipMemcpyHostToDevice));
    if (nb) HIP_CHECK(hipMemcpy(d_b_.ptr, up_b_.data(), sizeof(float) * nb, hipMemcpyHostToDevice));
    uploaded_ = true;
}

void LinearTransform::apply_device(idx_t n, const float* x, int ldx, float* xt, int ldxt,
                                   hipStream_t s) const {
    if (!uploaded_) sync_device();
    kern::linear_transform(x, n, ldx, d_A_.as<float>(), d_in, d_out,
                           have_bias ? d_b_.as<float>() : nullptr, xt, ldxt, s);
}

void LinearTransform::transpose_device(idx_t n, const float* y, int ldy, float* x, int ldx,
                                       hipStream_t s) const {
    if (!uploaded_) sync_device();
    kern::linear_transform_transposed(y, n, ldy, d_A_.as<float>(), d_in, d_out,
                                      have_bias ? d_b_.as<float>() : nullptr, x, ldx, s);
}

void LinearTransform::transform_transpose(idx_t n, const float* y, float* x) const {
    sync_device();
    host_pass(n, y, d_out, x, d_in,
              [&](idx_t nq, const float* a, int lda, float* o, int ldo, hipStream_t s) {
                  transpose_device(nq, a, lda, o, ldo, s);
              });
}

void LinearTransform::reverse_device(idx_t n, const float* xt, int ldxt, float* x, int ldx,
                                     hipStream_t s) const {
    FAISS_THROW_IF_NOT_MSG(is_orthonormal,
                           "reverse transform not implemented for non-orthonormal matrices");
    transpose_device(n, xt, ldxt, x, ldx, s);
}

void LinearTransform::reverse_transform(idx_t n, const float* xt, float* x) const {
    FAISS_THROW_IF_NOT_MSG(is_orthonormal,
                           "reverse transform not implemented for non-orthonormal matrices");
    transform_transpose(n, xt, x);
}

void LinearTransform::set_is_orthonormal() {
    // faiss/VectorTransform.cpp:240-284 (the reference's A^T A in column-major
    // terms is A A^T of the row-major [d_out][d_in] matrix)
    if (d_out > d_in) {
        is_orthonormal = false;
        return;
    }
    if (d_out == 0) {
        is_orthonormal = true;
        return;
    }
    const double eps = 4e-5;
    FAISS_THROW_IF_NOT(A.size() >= (size_t)d_out * d_in);
    is_orthonormal = true;
    for (int i = 0; i < d_out && is_orthonormal; i++)
        for (int j = 0; j <= i; j++) {
            float v = 0;
            const float *ai = A.data() + (size_t)i * d_in, *aj = A.data() + (size_t)j * d_in;
            for (int k = 0; k < d_in; k++) v += ai[k] * aj[k];
            if (i == j) v -= 1;
            if (std::fabs(v) > eps) {
                is_orthonormal = false;
                break;
            }
        }
}

// ---------------------------------------------------------------- named transforms
void RandomRotationMatrix::init(int) {
    FAISS_THROW_MSG("RandomRotationMatrix::init is not served (it needs the reference's QR); "
                    "read a trained transform or set A");
}
void RandomRotationMatrix::train(idx_t, const float*) {
    if (!is_trained) no_training("RandomRotationMatrix");
}

PCAMatrix::PCAMatrix(int d_in, int d_out, float eigen_power, bool random_rotation)
        : LinearTransform(d_in, d_out, true),
          eigen_power(eigen_power),
          random_rotation(random_rotation) {}
void PCAMatrix::train(idx_t, const float*) {
    if (!is_trained) no_training("PCAMatrix");
}

OPQMatrix::OPQMatrix(int d, int M, int d2) : LinearTransform(d, d2 == -1 ? d : d2, false), M(M) {}
void OPQMatrix::train(idx_t, const float*) {
    if (!is_trained) no_training("OPQMatrix");
}

// ---------------------------------------------------------------- IndexPreTransform
IndexPreTransform::IndexPreTransform() = default;

IndexPreTransform::IndexPreTransform(Index* idx) : Index(idx->d, idx->metric_type), index(idx) {
    device = idx->device;
    is_trained = idx->is_trained;
    ntotal = idx->ntotal;
}

IndexPreTransform::IndexPreTransform(VectorTransform* ltrans, Index* idx)
        : Index(idx->d, idx->metric_type), index(idx) {
    device = idx->device;
    is_trained = idx->is_trained;
    ntotal = idx->ntotal;
    prepend_transform(ltrans);
}

IndexPreTransform::~IndexPreTransform() {
    if (own_fields) {
        for (auto* t : chain) delete t;
        delete index;
    }
}

void IndexPreTransform::prepend_transform(VectorTransform* ltrans) {
    FAISS_THROW_IF_NOT(ltrans->d_out == d);
    is_trained = is_trained && ltrans->is_trained;
    chain.insert(chain.begin(), ltrans);
    d = ltrans->d_in;
    version_++;
}

void IndexPreTransform::train(idx_t n, const float* x) {
    // faiss/IndexPreTransform.cpp:66-121, without the transforms' own
    // training: an untrained one is asked, and the named ones throw
    FAISS_THROW_IF_NOT(index);
    for (auto* t : chain)
        if (!t->is_trained) {
            t->train(n, x);
            FAISS_THROW_IF_NOT_MSG(t->is_trained, "Transformation not trained yet");
        }
    if (!index->is_trained) {
        const float* xt = apply_chain(n, x);
        std::unique_ptr<const float[]> del(xt == x ? nullptr : xt);
        index->train(n, xt);
    }
    is_trained = true;
}

const float* IndexPreTransform::apply_chain(idx_t n, const float* x) const {
    if (chain.empty()) return x;
    std::unique_ptr<float[]> xt(new float[(size_t)n * index->d]);
    apply_chain_noalloc(n, x, xt.get());
    return xt.release();
}

void IndexPreTransform::apply_chain_noalloc(idx_t n, const float* x, float* xt) const {
    FAISS_THROW_IF_NOT(index);
    if (chain.empty()) {
        memcpy(xt, x, sizeof(float) * (size_t)n * d);
        return;
    }
    FAISS_THROW_IF_NOT(chain.back()->d_out == index->d);
    DevGuard dg(device);
    for (auto* t : chain) t->sync_device();
    hipStream_t s = stream();
    const int li = ld4(d), lo = index->ld();
    // the chunk holds the input, the result and the intermediate rows
    int widest = li + lo;
    for (auto* t : chain) widest = std::max(widest, ld4(t->d_in) + ld4(t->d_out));
    const idx_t qc = host_chunk(n, widest, 0);
    std::lock_guard<std::recursive_mutex> g(mu_);
    s_in_.reserve(sizeof(float) * qc * li);
    for (idx_t q0 = 0; q0 < n; q0 += qc) {
        const idx_t nq = std::min(qc, n - q0);
        upload_rows(s_in_.as<float>(), li, x + q0 * d, (int)d, nq, s);
        int ldxt = 0;
        order_.enter(s);
        const float* r = apply_chain_device(nq, s_in_.as<float>(), li, &ldxt, s);
        order_.leave(s);
        download_rows(xt + q0 * index->d, index->d, r, ldxt, nq, s);
    }
}

const float* IndexPreTransform::apply_chain_device(idx_t n, const float* x, int ldx, int* ldxt,
                                                   hipStream_t s) const {
    const float* cur = x;
    int ldc = ldx;
    for (size_t i = 0; i < chain.size(); i++) {
        const VectorTransform* t = chain[i];
        FAISS_THROW_IF_NOT_FMT(i == 0 ? t->d_in == d : t->d_in == chain[i - 1]->d_out,
                               "IndexPreTransform: transform %zu takes %d dimensions, not what "
                               "precedes it",
                               i, t->d_in);
        DeviceBuffer& out = (i & 1) ? s_t1_ : s_t0_;
        const int ldo = ld4(t->d_out);
        out.reserve(sizeof(float) * (size_t)n * ldo);
        t->apply_device(n, cur, ldc, out.as<float>(), ldo, s);
        cur = out.as<float>();
        ldc = ldo;
    }
    *ldxt = ldc;
    return cur;
}

void IndexPreTransform::reverse_chain(idx_t n, const float* xt, float* x) const {
    // faiss/IndexPreTransform.cpp:147-162
    const float* next_x = xt;
    std::unique_ptr<float[]> del;
    for (int i = (int)chain.size() - 1; i >= 0; i--) {
        const VectorTransform* t = chain[i];
        std::unique_ptr<float[]> prev;
        float* prev_x = x;
        if (i != 0) {
            prev.reset(new float[(size_t)n * t->d_in]);
            prev_x = prev.get();
        }
        t->reverse_transform(n, next_x, prev_x);
        del = std::move(prev);
        next_x = prev_x;
    }
    if (chain.empty()) memcpy(x, xt, sizeof(float) * (size_t)n * d);
}

namespace {
// faiss/IndexPreTransform.cpp:166-175
const SearchParameters* extract_index_search_params(const SearchParameters* params_in) {
    auto params = dynamic_cast<const SearchParametersPreTransform*>(params_in);
    return params ? params->index_params : params_in;
}
}  // namespace

void IndexPreTransform::add(idx_t n, const float* x) {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    std::unique_ptr<const float[]> del(xt == x ? nullptr : xt);
    index->add(n, xt);
    ntotal = index->ntotal;
    version_++;
}

void IndexPreTransform::add_with_ids(idx_t n, const float* x, const idx_t* xids) {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    std::unique_ptr<const float[]> del(xt == x ? nullptr : xt);
    index->add_with_ids(n, xt, xids);
    ntotal = index->ntotal;
    version_++;
}

void IndexPreTransform::reset() {
    index->reset();
    ntotal = 0;
    version_++;
}

size_t IndexPreTransform::remove_ids(const IDSelector& sel) {
    const size_t nremove = index->remove_ids(sel);
    ntotal = index->ntotal;
    version_++;
    return nremove;
}

void IndexPreTransform::sync_device() const {
    if (index) index->sync_device();
    for (auto* t : chain) t->sync_device();
}

void IndexPreTransform::fold_device_stats() const {
    if (index) index->fold_device_stats();
}

namespace {
struct Leave {
    StreamOrder& o;
    hipStream_t s;
    ~Leave() {
        try {
            o.leave(s);
        } catch (...) {
        }
    }
};
}  // namespace

void IndexPreTransform::search_device(idx_t n, const float* x, int ldx, idx_t k, float* distances,
                                      idx_t* labels, const SearchParameters* params,
                                      hipStream_t s) const {
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT(index);
    if (n == 0) return;
    const SearchParameters* bp = extract_index_search_params(params);
    if (chain.empty()) {
        index->search_device(n, x, ldx, k, distances, labels, bp, s);
        return;
    }
    FAISS_THROW_IF_NOT(chain.back()->d_out == index->d);
    DevGuard dg(device);
    std::lock_guard<std::recursive_mutex> g(mu_);
    order_.enter(s);
    Leave leave{order_, s};
    int widest = 4;
    for (auto* t : chain) widest = std::max(widest, ld4(t->d_out));
    const idx_t qc = host_chunk(n, widest, 0);  // rows per pass: 256 MiB per scratch buffer
    for (idx_t q0 = 0; q0 < n; q0 += qc) {
        const idx_t nq = std::min(qc, n - q0);
        int ldxt = 0;
        const float* xt;
        {
            ScopedKernelTimer tm(&ktimes, "pretransform", 2.0 * nq * d * index->d, s);
            xt = apply_chain_device(nq, x + q0 * ldx, ldx, &ldxt, s);
        }
        index->search_device(nq, xt, ldxt, k, distances + q0 * k, labels + q0 * k, bp, s);
    }
}

void IndexPreTransform::assign_device(idx_t n, const float* x, int ldx, int k, float* distances,
                                      int32_t* labels, const SearchParameters* params,
                                      hipStream_t s) const {
    FAISS_THROW_IF_NOT(index);
    if (n == 0) return;
    const SearchParameters* bp = extract_index_search_params(params);
    DevGuard dg(device);
    std::lock_guard<std::recursive_mutex> g(mu_);
    order_.enter(s);
    Leave leave{order_, s};
    int widest = 4;
    for (auto* t : chain) widest = std::max(widest, ld4(t->d_out));
    const idx_t qc = host_chunk(n, widest, 0);
    for (idx_t q0 = 0; q0 < n; q0 += qc) {
        const idx_t nq = std::min(qc, n - q0);
        int ldxt = 0;
        const float* xt = apply_chain_device(nq, x + q0 * ldx, ldx, &ldxt, s);
        index->assign_device(nq, xt, ldxt, k, distances + q0 * k, labels + q0 * k, bp, s);
    }
}

void IndexPreTransform::range_search(idx_t n, const float* x, float radius,
                                     RangeSearchResult* result,
                                     const SearchParameters* params) const {
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    std::unique_ptr<const float[]> del(xt == x ? nullptr : xt);
    index->range_search(n, xt, radius, result, extract_index_search_params(params));
}

void IndexPreTransform::reconstruct(idx_t key, float* recons) const {
    std::vector<float> tmp((size_t)index->d);
    index->reconstruct(key, tmp.data());
    reverse_chain(1, tmp.data(), recons);
}

void IndexPreTransform::reconstruct_n(idx_t i0, idx_t ni, float* recons) const {
    std::vector<float> tmp((size_t)ni * index->d);
    index->reconstruct_n(i0, ni, tmp.data());
    reverse_chain(ni, tmp.data(), recons);
}

void IndexPreTransform::search_and_reconstruct(idx_t n, const float* x, idx_t k, float* distances,
                                               idx_t* labels, float* recons,
                                               const SearchParameters* params) const {
    // faiss/IndexPreTransform.cpp:265-297
    FAISS_THROW_IF_NOT(k > 0);
    FAISS_THROW_IF_NOT(is_trained);
    const float* xt = apply_chain(n, x);
    std::unique_ptr<const float[]> del(xt == x ? nullptr : xt);
    const SearchParameters* bp = extract_index_search_params(params);
    std::vector<float> tmp((size_t)n * k * index->d);
    if (auto ivf = dynamic_cast<const IndexIVF*>(index)) {
        ivf->search_and_reconstruct(n, xt, k, distances, labels, tmp.data(), bp);
    } else {
        // faiss/Index.cpp:85-110
        index->search(n, xt, k, distances, labels, bp);
        for (idx_t i = 0; i < n * k; i++) {
            float* r = tmp.data() + (size_t)i * index->d;
            if (labels[i] < 0)
                memset(r, -1, sizeof(float) * index->d);
            else
                index->reconstruct(labels[i], r);
        }
    }
    reverse_chain(n * k, tmp.data(), recons);
}

// ---------------------------------------------------------------- extract_index_ivf
const IndexIVF* try_extract_index_ivf(const Index* index) {
    for (;;) {
        if (auto pt = dynamic_cast<const IndexPreTransform*>(index)) {
            index = pt->index;
        } else if (auto rf = dynamic_cast<const IndexRefine*>(index)) {
            index = rf->base_index;
        } else {
            break;
        }
    }
    return dynamic_cast<const IndexIVF*>(index);
}
IndexIVF* try_extract_index_ivf(Index* index) {
    return const_cast<IndexIVF*>(try_extract_index_ivf((const Index*)index));
}
const IndexIVF* extract_index_ivf(const Index* index) {
    const IndexIVF* ivf = try_extract_index_ivf(index);
    FAISS_THROW_IF_NOT(ivf);
    return ivf;
}
IndexIVF* extract_index_ivf(Index* index) {
    return const_cast<IndexIVF*>(extract_index_ivf((const Index*)index));
}

}  // namespace faiss_amd
