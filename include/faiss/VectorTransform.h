// faiss/VectorTransform.h — VectorTransform, LinearTransform and the named
// linear transforms (RandomRotationMatrix, PCAMatrix, OPQMatrix) as carriers
// of trained data.  They apply on the GPU; their training is not served and
// throws.  The other transform kinds of the reference are not declared.
#pragma once
#include "impl/faiss_amd_names.h"
