// faiss/IndexIVF.h — IndexIVF (with its DirectMap, remove_ids, update_vectors and the
// reconstruct family), SearchParametersIVF, IndexIVFStats, QueryLatencyStats
#pragma once
#include "impl/faiss_amd_names.h"
