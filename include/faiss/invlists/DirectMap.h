// faiss/invlists/DirectMap.h — DirectMap, lo_build / lo_listno / lo_offset
#pragma once
#include "../impl/faiss_amd_names.h"
