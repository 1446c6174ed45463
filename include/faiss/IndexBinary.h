// faiss/IndexBinary.h — the binary index classes (Hamming distance over bit vectors):
// IndexBinary, IndexBinaryFlat and IndexBinaryIVF, searched on the GPU.
#pragma once
#include "impl/faiss_amd_names.h"
