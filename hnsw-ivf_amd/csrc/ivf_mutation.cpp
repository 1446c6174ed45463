// ivf_mutation.cpp — editing an index and reading vectors back: DirectMap,
// remove_ids, update_vectors, reconstruct / reconstruct_n /
// reconstruct_from_offset and search_and_reconstruct.
//
// Reference: faiss/invlists/DirectMap.cpp, faiss/IndexIVF.cpp:287-297,
// :1407-1429, :1459-1512, :1594-1624, faiss/IndexFlatCodes.cpp:53-73,
// faiss/IndexIVFPQ.cpp:314-329, faiss/IndexScalarQuantizer.cpp:262-279.
//
// The host lists are authoritative.  A mutation marks the index dirty, so the
// next search packs and uploads the arena again and content_version() moves
// (captured search graphs retire); nothing is patched in HBM.
#include <algorithm>
#include <cstring>

#include "../../include/faiss_amd.h"
#include "kernels.h"
#include "sq_ref.h"

namespace faiss_amd {

namespace {
struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int dev) {
        ensure_hip();
        HIP_CHECK(hipGetDevice(&prev));
        if (prev != dev) HIP_CHECK(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        int cur = 0;
        hipGetDevice(&cur);
        if (cur != prev) hipSetDevice(prev);
    }
};
}  // namespace

// ---------------------------------------------------------------- Index
size_t Index::remove_ids(const IDSelector&) {
    FAISS_THROW_MSG("remove_ids not implemented for this type of index");  // faiss/Index.cpp:48
}

void Index::reconstruct_n(idx_t i0, idx_t ni, float* recons) const {
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    for (idx_t i = 0; i < ni; i++) reconstruct(i0 + i, recons + (size_t)i * d);
}

size_t IndexFlat::remove_ids(const IDSelector& sel) {
    idx_t j = 0;
    for (idx_t i = 0; i < ntotal; i++) {
        if (sel.is_member(i)) continue;
        if (i > j) memmove(xb.data() + (size_t)j * d, xb.data() + (size_t)i * d, sizeof(float) * d);
        j++;
    }
    const size_t nremove = (size_t)(ntotal - j);
    if (nremove > 0) {
        ntotal = j;
        xb.resize((size_t)ntotal * d);
        version_++;
        std::lock_guard<std::recursive_mutex> g(mu_);
        dirty_ = true;  // rows and norms are uploaded again
    }
    return nremove;
}

// ---------------------------------------------------------------- invlists
void ArrayInvertedLists::check_not_mapped(const char* what) const {
    if (!map) return;
    FAISS_THROW_MSG(std::string(what) + " is not possible on inverted lists mapped from " +
                    (map->name.empty() ? std::string("a file") : map->name) +
                    " (read-only mapping; ArrayInvertedLists::materialize() copies them to host "
                    "memory)");
}

void ArrayInvertedLists::update_entry(size_t l, size_t offset, idx_t id, const uint8_t* code) {
    check_not_mapped("update_entry");
    FAISS_THROW_IF_NOT(l < nlist && offset < ids[l].size());
    ids[l][offset] = id;
    memmove(codes[l].data() + offset * code_size, code, code_size);
}

void ArrayInvertedLists::resize(size_t l, size_t new_size) {
    check_not_mapped("resize");
    FAISS_THROW_IF_NOT(l < nlist);
    ids[l].resize(new_size);
    codes[l].resize(new_size * code_size);
}

// ---------------------------------------------------------------- DirectMap
void DirectMap::set_type(Type new_type, const ArrayInvertedLists* invlists, size_t ntotal) {
    FAISS_THROW_IF_NOT(new_type == NoMap || new_type == Array || new_type == Hashtable);
    if (new_type == type) return;
    array.clear();
    hashtable.clear();
    type = new_type;
    if (new_type == NoMap) return;
    if (new_type == Array)
        array.resize(ntotal, -1);
    else
        hashtable.reserve(ntotal);
    for (size_t key = 0; key < invlists->nlist; key++) {
        const size_t list_size = invlists->list_size(key);
        const idx_t* idlist = invlists->get_ids(key);
        for (size_t ofs = 0; ofs < list_size; ofs++) {
            if (new_type == Array) {
                FAISS_THROW_IF_NOT_MSG(0 <= idlist[ofs] && (size_t)idlist[ofs] < ntotal,
                                       "direct map supported only for seuquential ids");
                array[idlist[ofs]] = lo_build(key, ofs);
            } else {
                hashtable[idlist[ofs]] = lo_build(key, ofs);
            }
        }
    }
}

void DirectMap::clear() {
    array.clear();
    hashtable.clear();
}

idx_t DirectMap::get(idx_t key) const {
    if (type == Array) {
        FAISS_THROW_IF_NOT_MSG(key >= 0 && (size_t)key < array.size(), "invalid key");
        const idx_t lo = array[key];
        FAISS_THROW_IF_NOT_MSG(lo >= 0, "-1 entry in direct_map");
        return lo;
    } else if (type == Hashtable) {
        auto res = hashtable.find(key);
        FAISS_THROW_IF_NOT_MSG(res != hashtable.end(), "key not found");
        return res->second;
    }
    FAISS_THROW_MSG("direct map not initialized");
}

void DirectMap::add_single_id(idx_t id, idx_t list_no, size_t offset) {
    if (type == NoMap) return;
    if (type == Array) {
        FAISS_THROW_IF_NOT((size_t)id == array.size());
        array.push_back(list_no >= 0 ? lo_build(list_no, offset) : -1);
    } else if (list_no >= 0) {
        hashtable[id] = lo_build(list_no, offset);
    }
}

void DirectMap::check_can_add(const idx_t* ids) {
    if (type == Array && ids) FAISS_THROW_MSG("cannot have array direct map and add with ids");
}

size_t DirectMap::remove_ids(const IDSelector& sel, ArrayInvertedLists* invlists) {
    const size_t nlist = invlists->nlist;
    size_t nremove = 0;
    if (type == NoMap) {
        for (size_t i = 0; i < nlist; i++) {
            std::vector<idx_t>& ids = invlists->ids[i];
            uint8_t* codes = invlists->codes[i].data();
            const size_t cs = invlists->code_size;
            size_t l0 = ids.size(), l = l0, j = 0;
            while (j < l) {
                if (sel.is_member(ids[j])) {
                    l--;
                    ids[j] = ids[l];
                    memmove(codes + j * cs, codes + l * cs, cs);
                } else {
                    j++;
                }
            }
            if (l0 > l) {
                nremove += l0 - l;
                invlists->resize(i, l);
            }
        }
    } else if (type == Hashtable) {
        const IDSelectorArray* sela = dynamic_cast<const IDSelectorArray*>(&sel);
        FAISS_THROW_IF_NOT_MSG(sela, "remove with hashtable works only with IDSelectorArray");
        for (size_t i = 0; i < sela->n; i++) {
            auto res = hashtable.find(sela->ids[i]);
            if (res == hashtable.end()) continue;
            const size_t list_no = (size_t)lo_listno(res->second);
            const size_t offset = (size_t)lo_offset(res->second);
            const size_t last = invlists->list_size(list_no) - 1;
            hashtable.erase(res);
            if (offset < last) {
                const idx_t last_id = invlists->ids[list_no][last];
                invlists->update_entry(list_no, offset, last_id,
                                       invlists->codes[list_no].data() +
                                               last * invlists->code_size);
                hashtable[last_id] = lo_build(list_no, offset);
            }
            invlists->resize(list_no, last);
            nremove++;
        }
    } else {
        FAISS_THROW_MSG("remove not supported with this direct_map format");
    }
    return nremove;
}

void DirectMap::update_codes(ArrayInvertedLists* invlists, int n, const idx_t* ids,
                             const idx_t* assign, const uint8_t* codes) {
    FAISS_THROW_IF_NOT(type == Array);
    const size_t code_size = invlists->code_size;
    for (int i = 0; i < n; i++) {
        const idx_t id = ids[i];
        FAISS_THROW_IF_NOT_MSG(0 <= id && (size_t)id < array.size(), "id to update out of range");
        {  // remove the old entry
            const idx_t dm = array[id];
            FAISS_THROW_IF_NOT_MSG(dm >= 0, "-1 entry in direct_map");
            const size_t ofs = (size_t)lo_offset(dm), il = (size_t)lo_listno(dm);
            const size_t l = invlists->list_size(il);
            if (ofs != l - 1) {  // move l - 1 to ofs
                const idx_t id2 = invlists->ids[il][l - 1];
                array[id2] = lo_build(il, ofs);
                invlists->update_entry(il, ofs, id2,
                                       invlists->codes[il].data() + (l - 1) * code_size);
            }
            invlists->resize(il, l - 1);
        }
        {  // insert the new one
            const idx_t il = assign[i];
            FAISS_THROW_IF_NOT_MSG(il >= 0 && (size_t)il < invlists->nlist,
                                   "update_vectors: a vector the quantizer assigns to no list");
            array[id] = lo_build(il, invlists->list_size(il));
            invlists->add_entries(il, 1, &id, codes + (size_t)i * code_size);
        }
    }
}

// ---------------------------------------------------------------- IndexIVF
void IndexIVF::mark_mutated() {
    std::lock_guard<std::recursive_mutex> g(mu_);
    dirty_ = true;
    version_++;
}

void IndexIVF::make_direct_map(bool b) {
    direct_map().set_type(b ? DirectMap::Array : DirectMap::NoMap, invlists.get(), ntotal);
}

void IndexIVF::set_direct_map_type(DirectMap::Type type) {
    direct_map().set_type(type, invlists.get(), ntotal);
}

size_t IndexIVF::remove_ids(const IDSelector& sel) {
    invlists->check_not_mapped("remove_ids");
    const size_t nremove = direct_map().remove_ids(sel, invlists.get());
    ntotal -= nremove;
    if (nremove) mark_mutated();
    return nremove;
}

void IndexIVF::update_vectors(int n, const idx_t* new_ids, const float* x) {
    invlists->check_not_mapped("update_vectors");
    if (direct_map().type == DirectMap::Hashtable) {
        // just remove then add
        IDSelectorArray sel(n, new_ids);
        const size_t nremove = remove_ids(sel);
        FAISS_THROW_IF_NOT_MSG(nremove == (size_t)n, "did not find all entries to remove");
        add_with_ids(n, x, new_ids);
        mark_mutated();
        return;
    }
    FAISS_THROW_IF_NOT(direct_map().type == DirectMap::Array);
    FAISS_THROW_IF_NOT(is_trained);
    if (n <= 0) return;
    std::vector<idx_t> assign(n);
    std::vector<float> dis(n);
    quantizer->search(n, x, 1, dis.data(), assign.data());
    std::vector<uint8_t> flat_codes((size_t)n * code_size);
    encode_vectors(n, x, assign.data(), flat_codes.data());
    // (the lists change entry by entry: dirty even when an id is refused midway)
    struct Mark {
        IndexIVF* ix;
        ~Mark() { ix->mark_mutated(); }
    } mark{this};
    direct_map().update_codes(invlists.get(), n, new_ids, assign.data(), flat_codes.data());
}

void IndexIVF::reconstruct(idx_t key, float* recons) const {
    const idx_t lo = direct_map().get(key);
    reconstruct_from_offset(lo_listno(lo), lo_offset(lo), recons);
}

void IndexIVF::reconstruct_n(idx_t i0, idx_t ni, float* recons) const {
    FAISS_THROW_IF_NOT(ni == 0 || (i0 >= 0 && i0 + ni <= ntotal));
    for (size_t list_no = 0; list_no < nlist; list_no++) {
        const size_t list_size = invlists->list_size(list_no);
        const idx_t* idlist = invlists->get_ids(list_no);
        for (size_t offset = 0; offset < list_size; offset++) {
            const idx_t id = idlist[offset];
            if (!(id >= i0 && id < i0 + ni)) continue;
            reconstruct_from_offset((int64_t)list_no, (int64_t)offset,
                                    recons + (size_t)(id - i0) * d);
        }
    }
}

namespace {
const uint8_t* single_code(const IndexIVF* ix, int64_t list_no, int64_t offset) {
    FAISS_THROW_IF_NOT(list_no >= 0 && (size_t)list_no < ix->nlist);
    FAISS_THROW_IF_NOT(offset >= 0 && (size_t)offset < ix->invlists->list_size(list_no));
    return ix->invlists->get_codes(list_no) + (size_t)offset * ix->code_size;
}
}  // namespace

void IndexIVFFlat::reconstruct_from_offset(int64_t list_no, int64_t offset, float* recons) const {
    memcpy(recons, single_code(this, list_no, offset), code_size);
}

void ProductQuantizer::decode(const uint8_t* code, float* x) const {
    for (size_t m = 0; m < M; m++) {
        // PQDecoderGeneric: bits [m nbits, (m + 1) nbits) of the little-endian stream
        const size_t o = m * nbits, sh = o & 7;
        uint32_t v = code[o >> 3];
        if (sh + nbits > 8) v |= (uint32_t)code[(o >> 3) + 1] << 8;
        const size_t c = (v >> sh) & ((1u << nbits) - 1u);
        memcpy(x + m * dsub, centroids.data() + (m * ksub + c) * dsub, sizeof(float) * dsub);
    }
}

void IndexIVFPQ::reconstruct_from_offset(int64_t list_no, int64_t offset, float* recons) const {
    pq.decode(single_code(this, list_no, offset), recons);
    if (by_residual) {
        std::vector<float> centroid(d);
        quantizer->reconstruct(list_no, centroid.data());
        for (int i = 0; i < d; i++) recons[i] += centroid[i];
    }
}

void IndexIVFScalarQuantizer::reconstruct_from_offset(int64_t list_no, int64_t offset,
                                                      float* recons) const {
    sq.decode(single_code(this, list_no, offset), recons, 1);
    if (by_residual) {
        std::vector<float> centroid(d);
        quantizer->reconstruct(list_no, centroid.data());
        for (int i = 0; i < d; i++) recons[i] += centroid[i];
    }
}

// ---------------------------------------------------------------- device side
void IndexIVFFlat::recons_args(void* p) const {
    auto& a = *(kern::ReconsArgs*)p;
    a.kind = kern::RECONS_FLAT;
    a.stride = (int)(sizeof(float) * roundup((size_t)d, 4));
    a.by_residual = 0;  // rows are the vectors (faiss/IndexIVFFlat.cpp:37-39)
}

void IndexIVFPQ::recons_args(void* p) const {
    auto& a = *(kern::ReconsArgs*)p;
    a.kind = kern::RECONS_PQ;
    a.stride = device_code_stride();
    a.pq_cent = d_pq_.as<float>();
    a.M = (int)pq.M;
    a.dsub = (int)pq.dsub;
    a.nbits = (int)pq.nbits;
    a.cent = d_cent_.as<float>();
    a.ldcent = ld();
}

void IndexIVFScalarQuantizer::recons_args(void* p) const {
    auto& a = *(kern::ReconsArgs*)p;
    a.kind = sq.qtype == ScalarQuantizer::QT_fp16 ? kern::RECONS_SQFP16 : kern::RECONS_SQ8;
    a.stride = device_code_stride();
    a.trained = d_trained_.as<float>();
    a.cent = d_cent_.as<float>();
    a.ldcent = ld();
}

void IndexIVF::reconstruct_pairs_device(idx_t n, idx_t* labels, float* recons,
                                        hipStream_t s) const {
    if (n <= 0) return;
    sync_device();
    std::lock_guard<std::recursive_mutex> g(mu_);
    kern::ReconsArgs a;
    a.by_residual = by_residual ? 1 : 0;
    recons_args(&a);
    a.d = d;
    a.codes = d_codes_.as<uint8_t>();
    a.ids = d_ids_.as<int64_t>();
    a.list_off = d_list_off_.as<uint32_t>();
    a.list_len = d_list_len_.as<uint32_t>();
    a.nlist = (int)nlist;
    ScopedKernelTimer tm(&ktimes, "ivf_reconstruct", 0.0, s);
    kern::ivf_reconstruct_pairs(a, n, labels, recons, s);
}

void IndexIVF::search_and_reconstruct_device(idx_t n, const float* x, int ldx, idx_t k,
                                             float* distances, idx_t* labels, float* recons,
                                             const SearchParameters* params_in,
                                             hipStream_t s) const {
    const SearchParametersIVF* params = nullptr;
    if (params_in) {
        params = dynamic_cast<const SearchParametersIVF*>(params_in);
        FAISS_THROW_IF_NOT_MSG(params, "IndexIVF params have incorrect type");
    }
    // (nprobe read as IndexIVF::search_device reads it)
    const size_t np = std::min(nlist, params && params->nprobe ? params->nprobe : nprobe);
    FAISS_THROW_IF_NOT(np > 0);
    FAISS_THROW_IF_NOT(k > 0);
    if (n <= 0) return;
    const size_t mc = params ? params->max_codes : max_codes;
    DeviceGuard dg(device);
    sync_device();
    const uint8_t* sel = apply_selector(params, s);
    const idx_t qchunk = search_chunk(n, np, k);
    std::lock_guard<std::recursive_mutex> g(mu_);
    order_.enter(s);
    struct Leave {
        StreamOrder& o;
        hipStream_t s;
        ~Leave() { o.leave(s); }
    } leave{order_, s};
    s_cd_.reserve(sizeof(float) * qchunk * np);
    s_ci_.reserve(sizeof(int32_t) * qchunk * np);
    // per chunk: the coarse stage, the store_pairs scan (the general exact
    // scan, like every store_pairs search), then the rows
    for (idx_t q0 = 0; q0 < n; q0 += qchunk) {
        const idx_t nq = std::min(qchunk, n - q0);
        quantize_device(nq, x + q0 * ldx, ldx, (int)np, s_cd_.as<float>(), s_ci_.as<int32_t>(),
                        params ? params->quantizer_params : nullptr, s);
        const uint32_t* lim = nullptr;
        const int32_t* asg = apply_max_codes(nq, (int)np, s_ci_.as<int32_t>(), mc, &lim, s);
        search_preassigned_device(nq, x + q0 * ldx, ldx, k, (int)np, asg, s_cd_.as<float>(),
                                  distances + q0 * k, labels + q0 * k, s, lim, sel, true);
        reconstruct_pairs_device(nq * k, labels + q0 * k, recons + (size_t)q0 * k * d, s);
    }
}

void IndexIVF::search_and_reconstruct(idx_t n, const float* x, idx_t k, float* distances,
                                      idx_t* labels, float* recons,
                                      const SearchParameters* params) const {
    FAISS_THROW_IF_NOT(k > 0);
    if (n == 0) return;
    DeviceGuard dg(device);
    hipStream_t s = stream();
    const int ldx = ld();
    DeviceBuffer bx, bd, bi, br;
    bx.reserve(sizeof(float) * n * ldx);
    bd.reserve(sizeof(float) * n * k);
    bi.reserve(sizeof(idx_t) * n * k);
    br.reserve(sizeof(float) * n * k * d);
    if (ldx != d) HIP_CHECK(hipMemsetAsync(bx.ptr, 0, sizeof(float) * n * ldx, s));
    HIP_CHECK(hipMemcpy2DAsync(bx.ptr, sizeof(float) * ldx, x, sizeof(float) * d,
                               sizeof(float) * d, n, hipMemcpyHostToDevice, s));
    search_and_reconstruct_device(n, bx.as<float>(), ldx, k, bd.as<float>(), bi.as<idx_t>(),
                                  br.as<float>(), params, s);
    HIP_CHECK(hipMemcpyAsync(distances, bd.ptr, sizeof(float) * n * k, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(labels, bi.ptr, sizeof(idx_t) * n * k, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(recons, br.ptr, sizeof(float) * n * k * d, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    InterruptCallback::check();
}

}  // namespace faiss_amd
