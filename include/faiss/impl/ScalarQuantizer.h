// faiss/impl/ScalarQuantizer.h — ScalarQuantizer (QT_8bit / QT_fp16 ranges and codes)
#pragma once
#include "faiss_amd_names.h"
