// The identity in the `L` slot of a data set: `L = lensed_data ? LenseFlow : I` of load_nolensing_sim (src/dataset.jl:341-352), the operator of
// NoLensingDataSet, d = M B f + n (src/dataset.jl:37-47, 68-73).  Every action is a device copy (or nothing, in place); the identity has no phi,
// so a phi is accepted and ignored and there is no pullback with respect to it.  With it in the slot the composed paths of Dataset<T> compute the
// no-lensing model as they stand; on power-of-two maps Dataset<T> runs its flow-free fused forms instead (as_identity()).
#pragma once
#include "engine.hpp"

namespace cmbl {

template <typename T>
struct NoLens : LensOps<T> {
  Ctx<T>* c;
  explicit NoLens(Ctx<T>* ctx) : c(ctx) {}
  const char* op_name() const override { return "Identity"; }
  bool as_identity() const override { return true; }
  void op_check(int) const override {}
  void op_set_phi(int, const void*, int) override {}
  void op_lens(const T* in, T* out, int P, int B) override { c->copy_maps(in, out, (long)P * B); }
  void op_lens_F(T* in, T* ftil, cx<T>* F, int P, int B) override {
    if (ftil) c->copy_maps(in, ftil, (long)P * B);
    c->rfft2_F(in, F, (long)P * B);
  }
  bool op_has_adjoint() const override { return true; }
  void op_adj_F(const cx<T>* in, cx<T>* out, int P, int B) override {
    if (in != out) CMBL_HIP(hipMemcpyAsync(out, in, sizeof(cx<T>) * (long)P * B * c->plane(), hipMemcpyDeviceToDevice, c->stream));
  }
  bool op_has_inverse() const override { return true; }
  void op_inv(const T* in, T* out, int P, int B) override { c->copy_maps(in, out, (long)P * B); }
};

}  // namespace cmbl
