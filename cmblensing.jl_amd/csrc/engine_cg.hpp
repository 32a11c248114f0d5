// conjugate_gradient (src/numerical_algorithms.jl:73-134) with its scalars resident on the device, written once for every data set.  CgSolver<T> owns
// the vectors, the scalar block, the history and the host's view of the flags; a data set forms b and supplies the products.  begin<Block> ->
// (b into v.b) -> start -> one of the two forms of the iteration -> finish<Block>:
//   solve (CgStateBlock), any operator: two callables enqueue a product and leave its per-slot dot on the device,
//     A(const cx<T>* p, cx<T>* Ap, double* pAp_dev /*nullptr: no dot*/),  Pinv(const cx<T>* r, cx<T>* z, double* rz_dev);
//   solve_fused (CgScalBlock), power-of-two maps: one callable Ap(const cx<T>* p, cx<T>* Ap) -> DotOut leaves A p and returns the partials of p'Ap.
#pragma once
#include "engine.hpp"
#include "cg_host.hpp"

namespace cmbl {

// The host's view of a CG's device-resident flags: two pinned slots of up to 8 ints and an event each.  post: copy the flags after what has been
// enqueued and mark the point; wait: the flags as they were at that point, without draining the stream -- the host reads the stop flag of
// iteration i - 1 while iteration i runs.
struct CgFlagMirror {
  int* host = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  CgFlagMirror() = default;
  CgFlagMirror(const CgFlagMirror&) = delete; CgFlagMirror& operator=(const CgFlagMirror&) = delete;
  ~CgFlagMirror() { if (host) (void)hipHostFree(host); for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
  void ensure() {
    if (host) return;
    CMBL_HIP(hipHostMalloc((void**)&host, sizeof(int) * 16, hipHostMallocDefault));
    for (auto& e : ev) CMBL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  void post(int slot, const int* flags_dev, int nflag, hipStream_t stream) {
    CMBL_HIP(hipMemcpyAsync(host + 8 * slot, flags_dev, sizeof(int) * nflag, hipMemcpyDeviceToHost, stream));
    CMBL_HIP(hipEventRecord(ev[slot], stream));
  }
  const int* wait(int slot) { CMBL_HIP(hipEventSynchronize(ev[slot])); return host + 8 * slot; }
};

// The scalar block of a solve: ND x MAXBATCH doubles at sd, then 8 ints at si of which the first NFLAG are flags; NPOST of them go to the host
// after every iteration.  One definition per form of the iteration: where each scalar of its kernels' state lives, and which flag is which.
struct CgStateBlock {                                  // CgSolver::solve: CgState (kernels_pointwise.hpp), [MAXBATCH] each
  enum { ND = 6, NFLAG = 4, NPOST = 2, I_DONE = 0, I_NAN = 1, I_NH = 2, I_BETTER = 3 };
  static CgState carve(double* d, int* si, double* hist) {     // res, pAp, res2, alpha, beta, best
    return {d, d + MAXBATCH, d + 2 * MAXBATCH, d + 3 * MAXBATCH, d + 4 * MAXBATCH, d + 5 * MAXBATCH, hist, si + I_DONE, si + I_NAN, si + I_NH, si + I_BETTER};
  }
};
struct CgScalBlock {                                   // CgSolver::solve_fused: CgScal (kernels_harm.hpp); res, best, done, better are [2] by parity
  enum { ND = 7, NFLAG = 6, NPOST = 6, I_DONE = 0, I_BETTER = 2, I_NAN = 4, I_NH = 5 };
  static CgScal carve(double* sd, int* si, double* hist) { return {sd, sd + 2 * MAXBATCH, hist, si + I_DONE, si + I_BETTER, si + I_NAN, si + I_NH}; }
};

// fn(std::integral_constant<int, P>) for the P = 1, 2 or 3 polarisation planes of a field
template <typename Fn> void by_pol(int P, Fn&& fn) {
  if (P == 1) fn(std::integral_constant<int, 1>{}); else if (P == 2) fn(std::integral_constant<int, 2>{}); else fn(std::integral_constant<int, 3>{});
}

template <typename T>
struct CgSolver {
  Ctx<T>* c;
  DevBuf vec[7], scal, histb, rzfin;                   // x, r, z, p, Ap, the best x, b; grown on demand.  rzfin: r'z of every slot (solve_fused, B > 16)
  CgFlagMirror flags;                                  // pinned: [slot][up to 8 flags]
  // n complex elements over all B slots (nr reals per slot); sd, si: the scalar block (CgStateBlock / CgScalBlock); hist [maxit][B]
  struct Vecs { long n, nr; int B, maxit; cx<T>*x, *r, *z, *p, *Ap, *bx, *b; double* sd; int* si; double* hist; };
  explicit CgSolver(Ctx<T>* ctx) : c(ctx) {}
  template <typename Block> void post(const Vecs& v, int slot) { flags.post(slot, v.si, Block::NPOST, c->stream); }   // the flags as of what is enqueued
  template <typename Block> Vecs begin(long n, int B, int maxit) {
    Vecs v{n, 2 * n / B, B, maxit};
    cx<T>** const ptr[7] = {&v.x, &v.r, &v.z, &v.p, &v.Ap, &v.bx, &v.b};
    for (int i = 0; i < 7; ++i) { vec[i].ensure(sizeof(cx<T>) * n); *ptr[i] = vec[i].template as<cx<T>>(); }
    scal.ensure(sizeof(double) * Block::ND * MAXBATCH + sizeof(int) * 8);
    histb.ensure(sizeof(double) * (size_t)maxit * B);
    flags.ensure();
    v.sd = scal.template as<double>(); v.si = reinterpret_cast<int*>(v.sd + Block::ND * MAXBATCH); v.hist = histb.template as<double>();
    return v;
  }
  // x = fstart, r = b - A x;  or x = 0, r = b
  template <typename AF> void start(const Vecs& v, const cx<T>* fstart, AF&& A) {
    if (fstart) {
      CMBL_HIP(hipMemcpyAsync(v.x, fstart, sizeof(cx<T>) * v.n, hipMemcpyDeviceToDevice, c->stream));
      A(v.x, v.Ap, nullptr);
      std::vector<double> one(v.B, 1.0), mone(v.B, -1.0);
      c->lincomb((T*)v.r, (const T*)v.b, (const T*)v.Ap, one.data(), mone.data(), v.nr, v.B);
    } else {
      CMBL_HIP(hipMemsetAsync(v.x, 0, sizeof(cx<T>) * v.n, c->stream));
      CMBL_HIP(hipMemcpyAsync(v.r, v.b, sizeof(cx<T>) * v.n, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  // The iteration on CgState (kernels_pointwise.hpp; 6 doubles per slot): an iteration is enqueued without waiting for its reductions.
  template <typename AF, typename PF> void solve(const Vecs& v, AF&& A, PF&& Pinv, double tol) {
    const unsigned B = (unsigned)v.B, gx = (unsigned)std::min<long>((v.nr + NTP - 1) / NTP, 2048);
    const size_t bytes = sizeof(cx<T>) * v.n;
    T *x = (T*)v.x, *r = (T*)v.r, *p = (T*)v.p, *bx = (T*)v.bx;                 // (the vector kernels see complex arrays as reals)
    const T *z = (const T*)v.z, *Ap = (const T*)v.Ap;
    using Blk = CgStateBlock;
    CgState st = Blk::carve(v.sd, v.si, v.hist);
    hipStream_t sm = c->stream;
    Pinv(v.r, v.z, st.res);
    CMBL_HIP(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, sm));
    CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_start, dim3(1), 0, sm, st, v.B);
    CMBL_HIP(hipMemcpyAsync(bx, x, bytes, hipMemcpyDeviceToDevice, sm));
    post<Blk>(v, 0);
    if (flags.wait(0)[Blk::I_NAN] != 0) return;                              // a NaN start residual: finish reports it
    for (int it = 2; it <= v.maxit; ++it) {
      A(v.p, v.Ap, st.pAp);
      CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_alpha, dim3(1), 0, sm, st, v.B);
      CMBL_LAUNCH(c, K_CG, (k_cg_xr<T>), dim3(gx, B), 0, sm, x, r, (const T*)p, Ap, st, v.nr);
      Pinv(v.r, v.z, st.res2);
      CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_beta, dim3(1), 0, sm, st, v.B, tol);
      CMBL_LAUNCH(c, K_CG, (k_cg_p<T>), dim3(gx, B), 0, sm, p, z, st, v.nr);
      CMBL_LAUNCH(c, K_CG, (k_cg_keep_best<T>), dim3(gx), 0, sm, bx, (const T*)x, st, 2 * v.n);
      post<Blk>(v, it & 1);
      if (it > 2 && flags.wait((it - 1) & 1)[Blk::I_DONE] != 0) break;       // flags of the previous iteration
    }
  }
  // The fused form of the same iteration on CgScal (kernels_harm.hpp; power-of-two maps, P planes per slot, Pinv one harmonic operator): per iteration
  // Ap(p, Ap) and two flat launches (alpha; x, r, r'z -> beta and the stop test; p and the best iterate).  A sum is finished by the launch that consumes it.
  template <typename ApF> void solve_fused(const Vecs& v, int P, const OpRef<T>& Pinv, double tol, ApF&& Ap) {
    using Blk = CgScalBlock;
    const int B = v.B;
    rzfin.ensure(sizeof(double) * MAXBATCH);
    const CgScal st = Blk::carve(v.sd, v.si, v.hist);
    hipStream_t sm = c->stream;
    const ModeGeom<T> g = c->geom();
    const double sc = c->dot_scale();
    by_pol(P, [&](auto pp) {
      constexpr int PP = decltype(pp)::value;
      const DotOut o = c->pw_flat(PwCgStart<T, PP>{g, Pinv, v.x, v.r, v.p, v.bx}, B, Ctx<T>::PART_CG_RZ);
      CMBL_LAUNCH(c, K_CG, (k_cg_init<T>), dim3(1), 0, sm, st, o, sc, B);
    });
    post<Blk>(v, 0);
    if (flags.wait(0)[Blk::I_NAN] != 0) return;                              // a NaN start residual: finish reports it
    for (int it = 2, par = 0; it <= v.maxit; ++it, par ^= 1) {               // par: the parity the launches of this iteration read
      const DotOut oA = Ap(v.p, v.Ap);
      by_pol(P, [&](auto pp) {
        constexpr int PP = decltype(pp)::value;
        const DotOut oR = c->pw_flat(PwCgXr<T, PP>{g, Pinv, v.x, v.r, v.p, v.Ap, st, par, oA, sc}, B, Ctx<T>::PART_CG_RZ);   // alpha ; x, r
        // beta, stop test ; p, best iterate.  Every block needs r'z of ALL slots (`all(res < bestres)`, :111): up to 16 slots it adds
        // their partials itself in its prologue; beyond that one small launch finishes them first (O(B) instead of O(B^2) per block)
        const double* rzf = nullptr;
        if (B > 16) { double* const o1[1] = {rzfin.template as<double>()}; c->finish_parts(&oR, o1, 1, B); rzf = o1[0]; }
        c->pw_flat(PwCgP<T, PP>{g, Pinv, v.x, v.r, v.p, v.bx, st, par, tol, oR, sc, rzf}, B);
      });
      post<Blk>(v, it & 1);
      if (it > 2 && flags.wait((it - 1) & 1)[Blk::I_DONE + (it & 1)] != 0) break;   // previous iteration's flags: it left `done` at parity (it - 2) & 1
    }
  }
  // The best iterate to f_out; the flags of the block and the history come back behind one synchronise (cg_finish).  Returns the
  // length of the history; ERR_STATE for a length outside [0, maxit], ERR_NAN for a NaN residual.
  template <typename Block> int finish(const Vecs& v, cx<T>* f_out, double* hist) {
    hipStream_t sm = c->stream;
    int fl[Block::NFLAG];
    std::vector<double> hh((size_t)v.maxit * v.B);
    CMBL_HIP(hipMemcpyAsync(f_out, v.bx, sizeof(cx<T>) * v.n, hipMemcpyDeviceToDevice, sm));
    CMBL_HIP(hipMemcpyAsync(fl, v.si, sizeof(fl), hipMemcpyDeviceToHost, sm));
    CMBL_HIP(hipMemcpyAsync(hh.data(), v.hist, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, sm));
    CMBL_HIP(hipStreamSynchronize(sm));
    int nit = 0; std::string m;
    const int rc = cg_finish(fl, Block::NFLAG, Block::I_NAN, Block::I_NH, hh.data(), v.maxit, v.B, hist, &nit, m);
    if (rc) fail(rc, m);
    return nit;
  }
};

}  // namespace cmbl
