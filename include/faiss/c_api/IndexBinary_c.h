/*
 * IndexBinary_c.h — drop-in for the reference C API header
 * `c_api/IndexBinary_c.h`: the faiss_IndexBinary_* getters, train, add,
 * add_with_ids, search, reset, reconstruct and free, with the reference's
 * names, signatures and return codes (include/faiss_amd_c.h also declares the
 * constructors, casts, file functions and factory of the binary classes).
 */
#ifndef FAISS_INDEX_BINARY_C_H
#define FAISS_INDEX_BINARY_C_H

#include "faiss_c.h"

#endif /* FAISS_INDEX_BINARY_C_H */
