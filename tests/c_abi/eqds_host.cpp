// Stand-alone host program for the device-free logic of the ProjEquiRect data set (cmblensing.jl_amd/csrc/eqds_host.hpp: operator bookkeeping, the
// shape and state checks of the cmbl_eqds_* entry points) and of every CG solver (cg_host.hpp: the end of a solve, flags and history).  No HIP, no device, no Python: build
// it with the host sanitizers and run it on the CPU,
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/c_abi/eqds_host.cpp -o /tmp/eqds_host && /tmp/eqds_host
// (or hipcc -Xarch_host -fsanitize=address,undefined ...).  Exit status 0 and "eqds_host: ok" when every check holds.
#include "../../cmblensing.jl_amd/csrc/eqds_host.hpp"
#include "../../cmblensing.jl_amd/csrc/cg_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace cmbl;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "eqds_host: FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); } } while (0)

int main() {
  std::string msg;
  int dummy = 0;
  const void* blocks = &dummy;                                               // never dereferenced: the book keeps views

  // creation: npol, odd Nx with QU
  { EqdsBook b; CHECK(b.init(17, 30, 3, msg) == ERR_ARG); CHECK(b.init(17, 30, 0, msg) == ERR_ARG); }
  { EqdsBook b; CHECK(b.init(33, 45, 2, msg) == ERR_SHAPE); CHECK(b.init(33, 45, 1, msg) == OK); CHECK(b.n() == 33); }

  EqdsBook b;
  CHECK(b.init(17, 30, 2, msg) == OK && b.n() == 34);
  // nothing set: CF_INV is missing, whatever else is asked for
  CHECK(b.check(3, false, false, msg) == ERR_STATE && msg.find("CF_INV") != std::string::npos);
  // block operators: ids, sizes, what may be unset
  CHECK(b.set_block(-1, blocks, true, 34, msg) == ERR_ARG);
  CHECK(b.set_block(EQDS_NBLOCK, blocks, true, 34, msg) == ERR_ARG);
  CHECK(b.set_block(EQDS_CF_INV, blocks, true, 17, msg) == ERR_SHAPE);              // QU with n = Ny
  CHECK(!b.has(EQDS_CF_INV));
  CHECK(b.set_block(EQDS_CF_INV, blocks, true, 34, msg) == OK && b.has(EQDS_CF_INV) && b.blk[EQDS_CF_INV].cplx);
  CHECK(b.set_block(EQDS_CF_INV, nullptr, true, 34, msg) == ERR_ARG && b.has(EQDS_CF_INV));
  CHECK(b.set_block(EQDS_PRECOND_INV, nullptr, true, 34, msg) == ERR_ARG);
  CHECK(b.set_block(EQDS_B, blocks, false, 34, msg) == OK && b.has(EQDS_B) && !b.blk[EQDS_B].cplx);
  CHECK(b.set_block(EQDS_B, nullptr, false, 0, msg) == OK && !b.has(EQDS_B));      // unset: n is not looked at
  // the two forms of Cn^-1
  CHECK(b.check(3, false, false, msg) == OK);                                       // mean needs no Cn
  CHECK(b.check(3, true, false, msg) == ERR_STATE);                                 // none set
  CHECK(b.set_pixel(2, false, 1, msg) == ERR_ARG && b.set_pixel(-1, false, 1, msg) == ERR_ARG);
  CHECK(b.set_pixel(EQDS_CN_INV_PIX, false, 3, msg) == ERR_SHAPE && !b.cn_pix());
  b.dirty = false;
  CHECK(b.set_pixel(EQDS_CN_INV_PIX, false, 2, msg) == OK && b.cn_pix() && b.dirty);
  CHECK(b.check(3, true, false, msg) == OK);
  CHECK(b.set_block(EQDS_CN_INV, blocks, true, 34, msg) == OK);
  CHECK(b.check(3, true, false, msg) == ERR_STATE && msg.find("both") != std::string::npos);
  CHECK(b.set_pixel(EQDS_CN_INV_PIX, true, 0, msg) == OK && !b.cn_pix());           // unset: nplanes is not looked at
  CHECK(b.check(3, true, false, msg) == OK);
  CHECK(b.set_pixel(EQDS_MASK, false, 1, msg) == OK && b.pix_planes[EQDS_MASK] == 1);
  // the solver needs the preconditioner; nbatch in [1, 256]
  CHECK(b.check(3, true, true, msg) == ERR_STATE && msg.find("PRECOND_INV") != std::string::npos);
  CHECK(b.set_block(EQDS_PRECOND_INV, blocks, true, 34, msg) == OK && b.check(3, true, true, msg) == OK);
  CHECK(b.check(0, true, true, msg) == ERR_SHAPE && b.check(257, true, true, msg) == ERR_SHAPE && b.check(256, true, true, msg) == OK);

  // the end of a solve, for both layouts of the flag block (CgState: 4 ints, NaN at 1, length at 2; CgScal: 6 ints, NaN at 4, length at 5):
  // exactly nh * B residuals are copied, into a buffer of exactly that size (the sanitizer sees one element more)
  const int maxit = 8, B = 3;
  std::vector<double> dev((size_t)maxit * B);
  for (size_t i = 0; i < dev.size(); ++i) dev[i] = 1.0 / (double)(i + 1);
  const struct { int nflag, i_nan, i_nh; } layouts[2] = {{4, 1, 2}, {6, 4, 5}};
  for (const auto& l : layouts) {
    auto flags_of = [&](int nan, int nh) { std::vector<int> f((size_t)l.nflag, 1); f[l.i_nan] = nan; f[l.i_nh] = nh; return f; };   // every other flag set: not looked at
    auto finish = [&](const std::vector<int>& f, double* out, int* nit) { return cg_finish(f.data(), l.nflag, l.i_nan, l.i_nh, dev.data(), maxit, B, out, nit, msg); };
    for (int nh = 1; nh <= maxit; ++nh) {
      std::vector<double> out((size_t)nh * B, -1.0);
      int nit = -1;
      CHECK(finish(flags_of(0, nh), out.data(), &nit) == OK && nit == nh);
      for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == dev[i]);
    }
    {                                                                        // a NaN residual: the history is still handed over, the status says so
      std::vector<double> out((size_t)2 * B, -1.0);
      int nit = -1;
      CHECK(finish(flags_of(1, 2), out.data(), &nit) == ERR_NAN && nit == 2 && out[5] == dev[5]);
    }
    {                                                                        // a history length outside [0, maxit] copies nothing
      std::vector<double> out(1, -1.0);
      int nit = -1;
      CHECK(finish(flags_of(0, maxit + 1), out.data(), &nit) == ERR_STATE && out[0] == -1.0 && nit == -1);
      CHECK(finish(flags_of(0, -1), out.data(), &nit) == ERR_STATE && out[0] == -1.0 && nit == -1);
    }
  }
  {                                                                          // the indices must lie inside the flag block
    const int f[4] = {0, 0, 1, 0};
    double out[3]; int nit = -1;
    CHECK(cg_finish(f, 4, 4, 2, dev.data(), maxit, B, out, &nit, msg) == ERR_ARG && cg_finish(f, 4, 1, 5, dev.data(), maxit, B, out, &nit, msg) == ERR_ARG && nit == -1);
  }
  std::puts("eqds_host: ok");
  return 0;
}
