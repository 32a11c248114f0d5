// What Dataset<T> needs of a lensing operator in its `L` slot (load_sim(L = ...), src/dataset.jl:223, 306, 333): implemented by Flow<T>
// (LenseFlow, engine.hpp), Bilinear<T> (engine_bilinear.hpp), PowerLens<T> (PowerLens / Taylens, engine_powerlens.hpp) and NoLens<T> (the identity
// of load_nolensing_sim, engine_nolens.hpp).  Fields are in the
// internal layouts: maps [slice][x][y], Fourier planes in the F layout, QU.  An action the reference does not define for an operator is
// announced by its has_* member and refused with ERR_ARG by the default body: nothing is approximated.
#pragma once
#include "common.hpp"

namespace cmbl {

template <typename T> struct Flow;

template <typename T>
struct LensOps {
  virtual ~LensOps() = default;
  virtual const char* op_name() const = 0;
  // the LenseFlow behind this operator, for the fused forms of Dataset<T> that only it has; nullptr for every other operator
  virtual Flow<T>* as_flow() { return nullptr; }
  // true for NoLens<T> alone (L = I, src/dataset.jl:343): Dataset<T>::form is then FORM_IDENTITY, the flow-free forms (nolens_adjoint)
  virtual bool as_identity() const { return false; }
  // the operator has its phi (ERR_STATE otherwise) and takes B batch slots of f against it (ERR_SHAPE otherwise)
  virtual void op_check(int B) const = 0;
  // phi in the ABI's layout (basis MAP / FOURIER / HARMONIC), nb planes; the operators that refuse a batched phi fail with ERR_SHAPE
  virtual void op_set_phi(int basis, const void* phi, int nb) = 0;
  // out = L in over S = P B maps (in != out)
  virtual void op_lens(const T* in, T* out, int P, int B) = 0;
  // F = rfft2(L in).  ftil != nullptr (!= in): the lensed maps are left there as well; ftil == nullptr: `in` may be overwritten.  Hook of the
  // fused path: an operator may fold the lens into the column pass of the transform when the maps are not asked for (Bilinear<T>, option
  // "lens_fused"); otherwise the composition op_lens, rfft2_F
  virtual void op_lens_F(T* in, T* ftil, cx<T>* F, int P, int B) = 0;
  virtual bool op_has_adjoint() const { return false; }
  // out = rfft2(L' irfft2(in)), QU Fourier planes (in place allowed)
  virtual void op_adj_F(const cx<T>*, cx<T>*, int, int) { fail(ERR_ARG, std::string(op_name()) + ": the reference defines no adjoint of this operator"); }
  virtual bool op_has_pullback() const { return false; }
  // pullback of f~ = L f (src/flowops.jl:40-54, src/bilinearlens.jl:165-171): `ftil` the primal output (destroyed), `w` the cotangent in QU
  // Fourier (replaced by delta f = L' w), dphi: B planes.  alias_quirk is read by LenseFlow only
  virtual void op_pullback(T*, cx<T>*, cx<T>*, int, int, bool) { fail(ERR_ARG, std::string(op_name()) + ": the reference defines no pullback of L * f with respect to phi for this operator"); }
  virtual bool op_has_inverse() const { return false; }
  // out = L \ in over maps
  virtual void op_inv(const T*, T*, int, int) { fail(ERR_ARG, std::string(op_name()) + ": the reference defines no inverse of this operator"); }
};

}  // namespace cmbl
