// include/pbccs_amd/AlignMode.hpp -- ConsensusCore::AlignMode (Align/AlignConfig.hpp), shared by the POA facade
// (SparsePoa.hpp) and the pairwise aligners (Align.hpp).
#pragma once

#include "../pbccs_amd.h"

namespace ConsensusCore {

enum AlignMode { GLOBAL = PBCCS_POA_GLOBAL, SEMIGLOBAL = PBCCS_POA_SEMIGLOBAL, LOCAL = PBCCS_POA_LOCAL };

}  // namespace ConsensusCore
