// faiss/IndexScalarQuantizer.h — IndexScalarQuantizer and
// IndexIVFScalarQuantizer (QT_8bit / QT_fp16, d % 8 == 0) and
// faiss/impl/ScalarQuantizer.h.
#pragma once
#include "impl/faiss_amd_names.h"
