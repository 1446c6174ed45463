/*
 * Index_c.h — drop-in for the reference C API header `c_api/Index_c.h`
 * (Quaternijkon/hnsw-ivf = Faiss 1.10.0).  A C caller of the reference keeps
 * its `#include "Index_c.h"` (or <faiss/c_api/Index_c.h>) and links
 * libfaiss_amd.so: the declarations — Index: train / add / search / search_with_params / assign /
 * reconstruct / reconstruct_n / remove_ids / range_search / reset / free and the getters —
 * are this library's, with the reference's names, signatures and return codes
 * (include/faiss_amd_c.h, which cites each reference declaration).
 */
#ifndef FAISS_INDEX_C_H
#define FAISS_INDEX_C_H

#include "faiss_c.h"

#endif /* FAISS_INDEX_C_H */
