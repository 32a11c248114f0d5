// Host side of the fused column pass of a BilinearLens in a data set (kernels_lensop.hpp): Ctx<T>::y_lens, instantiated over CMBL_COL_LIST for both
// sources by tu_lensop_{f32,f64}.hip -- a translation unit of its own, so that the build time of the others does not move (api_decl.hpp has the map)
#pragma once
#include "engine.hpp"
#include "kernels_lensop.hpp"

namespace cmbl {

template <typename T>
void Ctx<T>::y_lens(bool transposed, const LensTab<T>& tab, const T* in, cx<T>* mixed, long slices) {
  CMBL_REQUIRE(!generic, ERR_STATE, "fused column pass called on the any-size path");
  CMBL_REQUIRE((long)Ny * Nx < (1L << 31), ERR_SHAPE, "map too large for the 32-bit pixel indices of the lensing table");
  const TileY t = tileY(slices, false);
  if (transposed) launch_col(K_LENS_Y, t, false, slices, stream, [](auto r, auto nt, auto lgm) { return k_y_lens<T, r(), nt(), lgm(), 1>; }, tab, in, mixed, twY.template as<cx<T>>(), Nx);
  else launch_col(K_LENS_Y, t, false, slices, stream, [](auto r, auto nt, auto lgm) { return k_y_lens<T, r(), nt(), lgm(), 0>; }, tab, in, mixed, twY.template as<cx<T>>(), Nx);
}

#define CMBL_INSTANTIATE_LENSOP(T) template void Ctx<T>::y_lens(bool, const LensTab<T>&, const T*, cx<T>*, long);

}  // namespace cmbl
