// conjugate_gradient (src/numerical_algorithms.jl:73-134) with its scalars resident on the device, written once for every data set.  CgSolver<T> owns
// the vectors, the scalar block, the history and the host's view of the flags; a data set forms b and supplies two callables that enqueue a product
// and leave its per-slot dot on the device:  A(const cx<T>* p, cx<T>* Ap, double* pAp_dev /*nullptr: no dot*/),  Pinv(const cx<T>* r, cx<T>* z, double* rz_dev).
// begin -> (b into v.b) -> start -> solve -> finish;  Dataset::wiener_cg_fused runs its own iteration (CgScal) between start and finish.
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

template <typename T>
struct CgSolver {
  Ctx<T>* c;
  DevBuf vec[7], scal, histb;                          // x, r, z, p, Ap, the best x, b; grown on demand
  CgFlagMirror flags;                                  // pinned: [slot][up to 8 flags]
  // n complex elements over all B slots (nr reals per slot); sd: nd doubles per slot x MAXBATCH, si: the 8 ints behind them; hist [maxit][B]
  struct Vecs { long n, nr; int B, maxit; cx<T>*x, *r, *z, *p, *Ap, *bx, *b; double* sd; int* si; double* hist; };
  explicit CgSolver(Ctx<T>* ctx) : c(ctx) {}
  Vecs begin(long n, int B, int maxit, int nd) {
    Vecs v{n, 2 * n / B, B, maxit};
    cx<T>** const ptr[7] = {&v.x, &v.r, &v.z, &v.p, &v.Ap, &v.bx, &v.b};
    for (int i = 0; i < 7; ++i) { vec[i].ensure(sizeof(cx<T>) * n); *ptr[i] = vec[i].template as<cx<T>>(); }
    scal.ensure(sizeof(double) * nd * MAXBATCH + sizeof(int) * 8);
    histb.ensure(sizeof(double) * (size_t)maxit * B);
    flags.ensure();
    v.sd = scal.template as<double>(); v.si = reinterpret_cast<int*>(v.sd + nd * MAXBATCH); v.hist = histb.template as<double>();
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
    double* const sd = v.sd;                                                 // res, pAp, res2, alpha, beta, best; hist; done, nan, nh, better
    CgState st{sd, sd + MAXBATCH, sd + 2 * MAXBATCH, sd + 3 * MAXBATCH, sd + 4 * MAXBATCH, sd + 5 * MAXBATCH, v.hist, v.si, v.si + 1, v.si + 2, v.si + 3};
    hipStream_t sm = c->stream;
    Pinv(v.r, v.z, st.res);
    CMBL_HIP(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, sm));
    CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_start, dim3(1), 0, sm, st, v.B);
    CMBL_HIP(hipMemcpyAsync(bx, x, bytes, hipMemcpyDeviceToDevice, sm));
    flags.post(0, st.done, 2, sm);
    if (flags.wait(0)[1] != 0) return;                                       // a NaN start residual: finish reports it
    for (int it = 2; it <= v.maxit; ++it) {
      A(v.p, v.Ap, st.pAp);
      CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_alpha, dim3(1), 0, sm, st, v.B);
      CMBL_LAUNCH(c, K_CG, (k_cg_xr<T>), dim3(gx, B), 0, sm, x, r, (const T*)p, Ap, st, v.nr);
      Pinv(v.r, v.z, st.res2);
      CMBL_LAUNCH_NT(c, K_CG, 64, k_cg_beta, dim3(1), 0, sm, st, v.B, tol);
      CMBL_LAUNCH(c, K_CG, (k_cg_p<T>), dim3(gx, B), 0, sm, p, z, st, v.nr);
      CMBL_LAUNCH(c, K_CG, (k_cg_keep_best<T>), dim3(gx), 0, sm, bx, (const T*)x, st, 2 * v.n);
      flags.post(it & 1, st.done, 2, sm);
      if (it > 2 && flags.wait((it - 1) & 1)[0] != 0) break;                 // flags of the previous iteration
    }
  }
  // The best iterate to f_out; the flags (nflag ints at flags_dev, see cg_finish) and the history come back behind one synchronise.  Returns the
  // length of the history; ERR_STATE for a length outside [0, maxit], ERR_NAN for a NaN residual.
  int finish(const Vecs& v, cx<T>* f_out, double* hist, const int* flags_dev, int nflag, int i_nan, int i_nh) {
    hipStream_t sm = c->stream;
    std::vector<int> fl((size_t)nflag);
    std::vector<double> hh((size_t)v.maxit * v.B);
    CMBL_HIP(hipMemcpyAsync(f_out, v.bx, sizeof(cx<T>) * v.n, hipMemcpyDeviceToDevice, sm));
    CMBL_HIP(hipMemcpyAsync(fl.data(), flags_dev, sizeof(int) * nflag, hipMemcpyDeviceToHost, sm));
    CMBL_HIP(hipMemcpyAsync(hh.data(), v.hist, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, sm));
    CMBL_HIP(hipStreamSynchronize(sm));
    int nit = 0; std::string m;
    const int rc = cg_finish(fl.data(), nflag, i_nan, i_nh, hh.data(), v.maxit, v.B, hist, &nit, m);
    if (rc) fail(rc, m);
    return nit;
  }
};

}  // namespace cmbl
