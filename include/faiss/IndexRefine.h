// faiss/IndexRefine.h — IndexRefine, IndexRefineFlat and
// IndexRefineSearchParameters.  The refine index is an IndexFlat on this path;
// any other refine index throws at construction, naming its type.
#pragma once
#include "impl/faiss_amd_names.h"
