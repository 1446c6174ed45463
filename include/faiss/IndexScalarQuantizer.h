// faiss/IndexScalarQuantizer.h — IndexIVFScalarQuantizer (QT_8bit / QT_fp16,
// d % 8 == 0) and faiss/impl/ScalarQuantizer.h.  The non-IVF
// IndexScalarQuantizer is not offered: code that names it does not compile.
#pragma once
#include "impl/faiss_amd_names.h"
