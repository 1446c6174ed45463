// faiss/IndexPreTransform.h — IndexPreTransform and
// SearchParametersPreTransform: a chain of linear transforms, applied on the
// GPU, in front of any index of this path.
#pragma once
#include "impl/faiss_amd_names.h"
