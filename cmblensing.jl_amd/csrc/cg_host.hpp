// The host-side end of a CG solve whose scalars live on the device (CgSolver::finish, engine_cg.hpp).  Plain C++, no HIP header, so that a
// stand-alone program can exercise it under the host sanitizers (tests/c_abi/eqds_host.cpp).
#pragma once
#include <string>
#include "status.hpp"

namespace cmbl {

// flags: the solver's nflag ints as the device left them, the NaN flag at i_nan and the length of the history at i_nh (CgState: 4 ints, 1 and 2;
// CgScal: 6 ints, 4 and 5).  hist_dev_copy: maxit * B doubles read back from the device.  The length is validated BEFORE it sizes a copy; then the
// nh recorded residual vectors go to hist_out, *nit is set and a NaN residual is reported (src/numerical_algorithms.jl:94).
inline int cg_finish(const int* flags, int nflag, int i_nan, int i_nh, const double* hist_dev_copy, int maxit, int B, double* hist_out, int* nit, std::string& msg) {
  if (i_nan < 0 || i_nan >= nflag || i_nh < 0 || i_nh >= nflag) { msg = "wiener_cg: flag index outside the flag block"; return ERR_ARG; }
  const int nh = flags[i_nh];
  if (nh < 0 || nh > maxit) { msg = "wiener_cg: corrupt history length"; return ERR_STATE; }
  for (long i = 0; i < (long)nh * B; ++i) hist_out[i] = hist_dev_copy[i];
  *nit = nh;
  if (flags[i_nan] != 0) { msg = "NaN residual in conjugate gradient"; return ERR_NAN; }
  return OK;
}

}  // namespace cmbl
