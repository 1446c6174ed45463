/*
 * IndexScalarQuantizer_c.h — drop-in for the reference C API header
 * `c_api/IndexScalarQuantizer_c.h` (Quaternijkon/hnsw-ivf = Faiss 1.10.0).  A C
 * caller of the reference keeps its `#include "IndexScalarQuantizer_c.h"` (or
 * <faiss/c_api/IndexScalarQuantizer_c.h>) and links libfaiss_amd.so: the
 * declarations — FaissQuantizerType and the IndexIVFScalarQuantizer constructors,
 * cast, destructor, getters and add_core — are this library's, with the
 * reference's names, signatures and return codes (include/faiss_amd_c.h, which
 * cites each reference declaration).  The non-IVF IndexScalarQuantizer functions
 * of the reference header are not declared: a caller of those fails to compile.
 */
#ifndef FAISS_INDEX_SCALAR_QUANTIZER_C_H
#define FAISS_INDEX_SCALAR_QUANTIZER_C_H

#include "faiss_c.h"

#endif /* FAISS_INDEX_SCALAR_QUANTIZER_C_H */
