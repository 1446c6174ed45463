// faiss/IndexPQ.h — IndexPQ, SearchParametersPQ and indexPQ_stats: the flat
// product-quantizer index (asymmetric search, nbits 4..8), searched on the GPU.
#pragma once
#include "impl/faiss_amd_names.h"
