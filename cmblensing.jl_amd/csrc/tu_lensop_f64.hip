// the fused column pass of a BilinearLens in a data set in double precision: k_y_lens (engine_lensop.hpp; api_decl.hpp has the map of the build)
#include "engine_lensop.hpp"
namespace cmbl { CMBL_INSTANTIATE_LENSOP(double) }
