/*
 * IndexPreTransform_c.h — drop-in for the reference C API header
 * `c_api/IndexPreTransform_c.h`: constructors, cast, destructor, the index and
 * own_fields accessors and prepend_transform, with the reference's names,
 * signatures and return codes (include/faiss_amd_c.h, which cites each
 * reference declaration).
 */
#ifndef FAISS_INDEX_PRETRANSFORM_C_H
#define FAISS_INDEX_PRETRANSFORM_C_H

#include "faiss_c.h"
#include "VectorTransform_c.h"

#endif /* FAISS_INDEX_PRETRANSFORM_C_H */
