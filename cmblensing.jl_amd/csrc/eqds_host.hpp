// Host-side bookkeeping of EqDataset<T> (engine_equirect_ds.hpp) that touches no device: which operators are set, and the shape and state checks
// of the entry points.  Plain C++, no HIP header, so that a stand-alone program can exercise it under the host sanitizers
// (tests/c_abi/eqds_host.cpp, which also covers the end of a solve, cg_host.hpp).  The codes are cmbl::Status (status.hpp).
#pragma once
#include <string>
#include "status.hpp"

namespace cmbl {

enum { EQDS_CF_INV = 0, EQDS_B = 1, EQDS_PRECOND_INV = 2, EQDS_CN_INV = 3, EQDS_NBLOCK = 4 };   // CMBL_EQDS_* block operators
enum { EQDS_MASK = 0, EQDS_CN_INV_PIX = 1, EQDS_NPIXOP = 2 };                                    // CMBL_EQDS_* map-diagonal operators

struct EqdsBook {
  int Ny = 0, Nx = 0, P = 0;
  struct Block { const void* p = nullptr; bool cplx = false; } blk[EQDS_NBLOCK];   // non-owning views: the caller keeps the arrays alive
  int pix_planes[EQDS_NPIXOP] = {0, 0};                                            // 0: not set
  bool dirty = true;                                                               // the precombined data-space weights are out of date

  int n() const { return P * Ny; }
  int init(int Ny_, int Nx_, int npol, std::string& msg) {
    if (npol != 1 && npol != 2) { msg = "eqds_create: npol must be 1 (spin 0) or 2 (spin 2); IQUAzFourier has no transform in the reference"; return ERR_ARG; }
    if (npol == 2 && Nx_ % 2) { msg = "eqds_create: QUAzFourier needs an even Nx (src/proj_equirect.jl:166)"; return ERR_SHAPE; }
    Ny = Ny_; Nx = Nx_; P = npol;
    return OK;
  }
  int set_block(int which, const void* p, bool cplx, int n_, std::string& msg) {
    if (which < 0 || which >= EQDS_NBLOCK) { msg = "eqds_set_block_op: bad operator id"; return ERR_ARG; }
    if (!p) {
      if (which != EQDS_B && which != EQDS_CN_INV) { msg = "eqds_set_block_op: only B and CN_INV can be unset"; return ERR_ARG; }
      blk[which] = Block{};
      return OK;
    }
    if (n_ != n()) { msg = "eqds_set_block_op: n must be Ny for a spin-0 and 2 Ny for a spin-2 data set"; return ERR_SHAPE; }
    blk[which].p = p; blk[which].cplx = cplx;
    return OK;
  }
  int set_pixel(int which, bool unset, int nplanes, std::string& msg) {
    if (which < 0 || which >= EQDS_NPIXOP) { msg = "eqds_set_pixel_op: bad operator id"; return ERR_ARG; }
    if (!unset && nplanes != 1 && nplanes != P) { msg = "eqds_set_pixel_op: one plane, or one per polarisation"; return ERR_SHAPE; }
    pix_planes[which] = unset ? 0 : nplanes;
    dirty = true;
    return OK;
  }
  bool has(int which) const { return blk[which].p != nullptr; }
  bool cn_pix() const { return pix_planes[EQDS_CN_INV_PIX] > 0; }
  // what an evaluation needs: Cf^-1 and exactly one form of Cn^-1 (the solver: the preconditioner as well); nbatch in [1, 256]
  int check(int nbatch, bool need_cn, bool need_precond, std::string& msg) const {
    if (nbatch < 1 || nbatch > MAXBATCH) { msg = "eqds: nbatch must lie in [1, 256]"; return ERR_SHAPE; }
    if (!has(EQDS_CF_INV)) { msg = "eqds: the operator CF_INV has not been set"; return ERR_STATE; }
    if (need_cn && has(EQDS_CN_INV) && cn_pix()) { msg = "eqds: both forms of Cn^-1 are set (CN_INV and CN_INV_PIX): unset one"; return ERR_STATE; }
    if (need_cn && !has(EQDS_CN_INV) && !cn_pix()) { msg = "eqds: no form of Cn^-1 has been set (CN_INV or CN_INV_PIX)"; return ERR_STATE; }
    if (need_precond && !has(EQDS_PRECOND_INV)) { msg = "eqds: the operator PRECOND_INV has not been set"; return ERR_STATE; }
    return OK;
  }
};

}  // namespace cmbl
