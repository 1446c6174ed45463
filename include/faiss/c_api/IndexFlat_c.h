/*
 * IndexFlat_c.h — drop-in for the reference C API header `c_api/IndexFlat_c.h`
 * (Quaternijkon/hnsw-ivf = Faiss 1.10.0).  A C caller of the reference keeps
 * its `#include "IndexFlat_c.h"` (or <faiss/c_api/IndexFlat_c.h>) and links
 * libfaiss_amd.so: the declarations — IndexFlat / IndexFlatL2 / IndexFlatIP: constructors, xb, casts,
 * destructors; IndexRefineFlat: constructor, cast, destructor, own_fields and
 * k_factor —
 * are this library's, with the reference's names, signatures and return codes
 * (include/faiss_amd_c.h, which cites each reference declaration).
 */
#ifndef FAISS_INDEX_FLAT_C_H
#define FAISS_INDEX_FLAT_C_H

#include "faiss_c.h"

#endif /* FAISS_INDEX_FLAT_C_H */
