/*
 * VectorTransform_c.h — drop-in for the reference C API header
 * `c_api/VectorTransform_c.h`.  A C caller of the reference keeps its
 * `#include "VectorTransform_c.h"` (or <faiss/c_api/VectorTransform_c.h>) and
 * links libfaiss_amd.so: the declarations are this library's, with the
 * reference's names, signatures and return codes (include/faiss_amd_c.h, which
 * cites each reference declaration).  Linear transforms are served; the
 * constructors of the other kinds (ITQ, RemapDimensions, Normalization,
 * Centering) and the training of PCA / OPQ / random rotations return the
 * FaissException code.
 */
#ifndef FAISS_VECTOR_TRANSFORM_C_H
#define FAISS_VECTOR_TRANSFORM_C_H

#include "faiss_c.h"

#endif /* FAISS_VECTOR_TRANSFORM_C_H */
