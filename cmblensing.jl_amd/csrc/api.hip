// C ABI of libcmblens_hip.so (see include/cmblens.h): entry points, argument checks and error plumbing.  No kernel and no typed class is
// instantiated in this translation unit: an entry point calls a virtual member of the precision-free object its handle owns, or BY_DTYPE(ctx,
// do_x, args...) for a typed body of api_body.hpp, which tu_main_{f32,f64}.hip compile (api_decl.hpp has the map and the list of bodies).
#include "api_decl.hpp"

namespace cmbl { thread_local std::string g_last_error; }
using namespace cmbl;

// Driver scratch lives in the dataset, keyed by the flow it was built for (it holds a Flow<T>&): a flow that goes away must take its
// entries with it -- the buffers would otherwise leak until the dataset is destroyed, and a NEW flow allocated at the same address would
// silently inherit scratch built around the old one.  Datasets register here so that cmbl_lenseflow_destroy can find them.
static std::mutex g_ds_mtx;
static std::vector<cmbl_dataset*> g_datasets;
static void registry_add(cmbl_dataset* d) { std::lock_guard<std::mutex> l(g_ds_mtx); g_datasets.push_back(d); }
static void registry_remove(cmbl_dataset* d) { std::lock_guard<std::mutex> l(g_ds_mtx); g_datasets.erase(std::remove(g_datasets.begin(), g_datasets.end(), d), g_datasets.end()); }
static void registry_drop_flow(const FlowApi* f) { std::lock_guard<std::mutex> l(g_ds_mtx); for (cmbl_dataset* d : g_datasets) d->drv.erase(f); }

template <typename F>
static int guard(F&& f) {
  try { f(); return CMBL_OK; }
  catch (const Error& e) { g_last_error = e.msg; return e.code; }
  catch (const std::exception& e) { g_last_error = e.what(); return CMBL_ERR_ARG; }
  catch (...) { g_last_error = "unknown error"; return CMBL_ERR_ARG; }
}
#define NOTNULL(p) CMBL_REQUIRE((p) != nullptr, ERR_ARG, "null pointer argument: " #p)
#define BASIS_OK(b) CMBL_REQUIRE((b) >= 0 && (b) <= 2, ERR_ARG, "bad basis: " #b)
#define POLB_OK(P, B) CMBL_REQUIRE((P) >= 1 && (P) <= 3 && (B) >= 1, ERR_SHAPE, "npol must be 1..3 and nbatch >= 1")
#define SAME_CTX(ds, L) CMBL_REQUIRE((ds)->ctx == (L)->ctx, ERR_ARG, "dataset and flow belong to different contexts")
#define SAME_CTX_OP(ds, L) CMBL_REQUIRE((ds)->ctx == (L)->ctx, ERR_ARG, "the data set and the lensing operator belong to different contexts")

// a typed, non-owning view of an operator handle (cmbl_lensop_from_*)
template <typename H> static int lensop_view(H* L, int kind, cmbl_lensop** out) {
  return guard([&] {
    NOTNULL(L); NOTNULL(out);
    *out = new cmbl_lensop{L->ctx, kind, L};
  });
}

#ifdef CMBL_STAMPS
#define CMBL_STAMPS_UNITS(X) X(main_f32) X(main_f64) X(gen_f32) X(gen_f64) X(small_f32) X(small_f64) X(cty_f32_a) X(cty_f32_b) X(cty_f64_a) X(cty_f64_b) \
    X(ctx_f32_a) X(ctx_f32_b) X(ctx_f64_a) X(ctx_f64_b)
namespace cmbl {
#define CMBL_X(unit) int stamps_read_##unit(unsigned long long* out_host, int n);
CMBL_STAMPS_UNITS(CMBL_X)
#undef CMBL_X
}
#endif
extern "C" {

const char* cmbl_last_error(void) { return g_last_error.c_str(); }
int cmbl_version(void) { return 100; }
int cmbl_abi_version(void) { return CMBL_ABI_VERSION; }

int cmbl_ctx_create(int Ny, int Nx, double theta, int dtype, int device, void* stream, cmbl_ctx** out) {
  return guard([&] {
    NOTNULL(out);
    CMBL_REQUIRE(dtype == CMBL_F32 || dtype == CMBL_F64, ERR_ARG, "dtype must be CMBL_F32 or CMBL_F64");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) fail(ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    CMBL_REQUIRE(device >= 0 && device < ndev, ERR_ARG, "device index out of range");
    auto h = std::make_unique<cmbl_ctx>();
    BY_DTYPE_CODE(dtype, do_ctx_create, h.get(), Ny, Nx, theta, device, stream);
    *out = h.release();
  });
}
int cmbl_ctx_destroy(cmbl_ctx* ctx) { return guard([&] { delete ctx; }); }
int cmbl_ctx_synchronize(cmbl_ctx* ctx) { return guard([&] { NOTNULL(ctx); CMBL_HIP(hipStreamSynchronize(ctx->p->stream)); }); }

int cmbl_ctx_set_option(cmbl_ctx* ctx, const char* name, int value) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(name);
    int* o = ctx->p->opt_ptr(name);
    CMBL_REQUIRE(o != nullptr, ERR_ARG, std::string("unknown option: ") + name);
    *o = value;
  });
}
int cmbl_ctx_get_option(cmbl_ctx* ctx, const char* name, int* value_host) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(name); NOTNULL(value_host);
    int* o = ctx->p->opt_ptr(name);
    CMBL_REQUIRE(o != nullptr, ERR_ARG, std::string("unknown option: ") + name);
    *value_host = *o;
  });
}
int cmbl_prof_enable(cmbl_ctx* ctx, int on) {
  return guard([&] { NOTNULL(ctx); if (!on) ctx->p->prof_collect(); ctx->p->prof_on = on != 0; });
}
int cmbl_prof_reset(cmbl_ctx* ctx) { return guard([&] { NOTNULL(ctx); ctx->p->prof_collect(); ctx->p->prof_reset(); }); }
int cmbl_prof_count(void) { return K_COUNT; }
const char* cmbl_prof_name(int k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }
int cmbl_prof_get(cmbl_ctx* ctx, int k, double* total_ms, long* launches) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(total_ms); NOTNULL(launches);
    CMBL_REQUIRE(k >= 0 && k < K_COUNT, ERR_ARG, "bad kernel class");
    ctx->p->prof_collect();
    *total_ms = ctx->p->prof_ms[k]; *launches = ctx->p->prof_n[k];
  });
}

int cmbl_timer_report(cmbl_ctx* ctx, char* buf, size_t buflen) {
  int need = 0;
  const int rc = guard([&] {
    NOTNULL(ctx);
    ctx->p->prof_collect();
    std::string r = "kernel_class launches total_ms mean_us\n";
    for (int k = 0; k < K_COUNT; ++k) {
      if (!ctx->p->prof_n[k]) continue;
      char line[160];
      std::snprintf(line, sizeof line, "%s %ld %.6f %.3f\n", kKernelNames[k], ctx->p->prof_n[k], ctx->p->prof_ms[k], 1e3 * ctx->p->prof_ms[k] / ctx->p->prof_n[k]);
      r += line;
    }
    need = (int)r.size();
    if (buf && buflen) { const size_t m = std::min(buflen - 1, r.size()); std::memcpy(buf, r.data(), m); buf[m] = 0; }
  });
  return rc == CMBL_OK ? need : -rc;
}
int cmbl_device_malloc(cmbl_ctx* ctx, size_t bytes, void** out) {
  return guard([&] { NOTNULL(ctx); NOTNULL(out); CMBL_HIP(hipSetDevice(ctx->p->device)); hipError_t e = hipMalloc(out, bytes); if (e != hipSuccess) { *out = nullptr; (void)hipGetLastError(); fail(ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e)); } });
}
int cmbl_device_free(cmbl_ctx* ctx, void* p) { return guard([&] { NOTNULL(ctx); CMBL_HIP(hipSetDevice(ctx->p->device)); if (p) CMBL_HIP(hipFree(p)); }); }
int cmbl_copy_to_device(cmbl_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(dst); NOTNULL(src);
    CMBL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->p->stream)); CMBL_HIP(hipStreamSynchronize(ctx->p->stream));
  });
}
int cmbl_copy_to_host(cmbl_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(dst); NOTNULL(src);
    CMBL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->p->stream)); CMBL_HIP(hipStreamSynchronize(ctx->p->stream));
  });
}

int cmbl_ctx_geometry_host(cmbl_ctx* ctx, int which, double* out, size_t n) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    const CtxBase& c = *ctx->p;
    const std::vector<double>* v = which == 0 ? &c.h_lx : which == 1 ? &c.h_ly : which == 2 ? &c.h_lam : which == 3 ? &c.h_sin2
                                 : which == 4 ? &c.h_cos2 : which == 5 ? &c.h_lmag : nullptr;
    CMBL_REQUIRE(v != nullptr, ERR_ARG, "bad geometry selector");
    CMBL_REQUIRE(n == v->size(), ERR_SHAPE, "geometry output has the wrong length");
    std::memcpy(out, v->data(), n * sizeof(double));
  });
}


int cmbl_convert(cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    BY_DTYPE(ctx, do_convert, ctx, bi, in, bo, out, P, B);
  });
}
int cmbl_rfft(cmbl_ctx* ctx, const void* map, void* fourier, int P, int B) { return cmbl_convert(ctx, CMBL_MAP, map, CMBL_FOURIER, fourier, P, B); }
int cmbl_irfft(cmbl_ctx* ctx, const void* fourier, void* map, int P, int B) { return cmbl_convert(ctx, CMBL_FOURIER, fourier, CMBL_MAP, map, P, B); }


int cmbl_diag_apply(cmbl_ctx* ctx, int kind, int bd, const void* diag, int bi, const void* in, int bo, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(diag); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    CMBL_REQUIRE(kind == CMBL_DIAG_MUL || kind == CMBL_DIAG_DIV_NAN2ZERO, ERR_ARG, "kind must be CMBL_DIAG_MUL or CMBL_DIAG_DIV_NAN2ZERO");
    CMBL_REQUIRE(bd == CMBL_FOURIER || bd == CMBL_HARMONIC, ERR_ARG, "operator must be diagonal in FOURIER or HARMONIC");
    BY_DTYPE(ctx, do_diag, ctx, kind, bd, diag, P, false, bi, in, bo, out, P, B);
  });
}
int cmbl_blockdiag_ieb_apply(cmbl_ctx* ctx, const void* te_bb, int transpose, int bi, const void* in, int bo, void* out, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(te_bb); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(3, B);
    BY_DTYPE(ctx, do_diag, ctx, 2, B_HARMONIC, te_bb, 5, transpose != 0, bi, in, bo, out, 3, B);
  });
}

int cmbl_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int P, int B, double* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(a); NOTNULL(b); NOTNULL(out); BASIS_OK(basis); POLB_OK(P, B);
    BY_DTYPE(ctx, do_dot, ctx, basis, a, b, P, B, out);
  });
}
int cmbl_norm(cmbl_ctx* ctx, int basis, const void* a, int P, int B, double* out) {
  const int rc = cmbl_dot(ctx, basis, a, a, P, B, out);
  if (rc == CMBL_OK) for (int i = 0; i < B; ++i) out[i] = std::sqrt(out[i]);
  return rc;
}
int cmbl_logdet_diag(cmbl_ctx* ctx, int basis, const void* d, int P, int B, double* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(d); NOTNULL(out); BASIS_OK(basis); POLB_OK(P, B);
    BY_DTYPE(ctx, do_diag_reduce, ctx, 0, basis, d, P, B, out);
  });
}
int cmbl_tr_diag(cmbl_ctx* ctx, int basis, const void* d, int P, int B, double* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(d); NOTNULL(out); BASIS_OK(basis); POLB_OK(P, B);
    BY_DTYPE(ctx, do_diag_reduce, ctx, 1, basis, d, P, B, out);
  });
}
int cmbl_set_sum_accuracy_mode(cmbl_ctx* ctx, int mode) {
  return guard([&] {
    NOTNULL(ctx);
    CMBL_REQUIRE(mode == CMBL_SUM_WORKING || mode == CMBL_SUM_FLOAT64 || mode == CMBL_SUM_KAHAN, ERR_ARG, "mode must be CMBL_SUM_WORKING, _FLOAT64 or _KAHAN");
    ctx->p->sum_mode = mode;
  });
}
int cmbl_logdet(cmbl_ctx* ctx, const void* d, int nplanes, double* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(d); NOTNULL(out); CMBL_REQUIRE(nplanes >= 1, ERR_ARG, "nplanes >= 1");
    BY_DTYPE(ctx, do_logdet, ctx, d, nplanes, out);
  });
}

// ---- LenseFlow -------------------------------------------------------------------------------------
int cmbl_lenseflow_create(cmbl_ctx* ctx, int nsteps, cmbl_flow** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    auto h = std::make_unique<cmbl_flow>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_flow_create, h.get(), nsteps);
    *out = h.release();
  });
}
int cmbl_lenseflow_destroy(cmbl_flow* L) { return guard([&] { if (L) registry_drop_flow(L->p.get()); delete L; }); }
int cmbl_lenseflow_set_phi(cmbl_flow* L, int basis, const void* phi, int nb) {
  return guard([&] {
    NOTNULL(L); NOTNULL(phi); BASIS_OK(basis); CMBL_REQUIRE(nb >= 1, ERR_SHAPE, "nbatch_phi >= 1");
    L->p->set_phi(basis, phi, nb);
  });
}
int cmbl_lenseflow_apply(cmbl_flow* L, int mode, int bi, const void* in, int bo, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(L); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    CMBL_REQUIRE(mode >= 0 && mode <= 3, ERR_ARG, "bad flow mode");
    L->p->apply(mode, bi, in, bo, out, P, B);
  });
}
int cmbl_lenseflow_grad(cmbl_flow* L, int mode, const void* f_end, int bdel, const void* delta, void* dphi, int bdf, void* df,
                        void* f_start, int P, int B, int quirk) {
  return guard([&] {
    NOTNULL(L); NOTNULL(f_end); NOTNULL(delta); NOTNULL(dphi); NOTNULL(df); BASIS_OK(bdel); BASIS_OK(bdf); POLB_OK(P, B);
    CMBL_REQUIRE(mode == CMBL_FLOW_FWD || mode == CMBL_FLOW_INV, ERR_ARG, "grad mode must be CMBL_FLOW_FWD or CMBL_FLOW_INV");
    L->p->grad(mode, f_end, bdel, delta, dphi, bdf, df, f_start, P, B, quirk != 0);
  });
}

int cmbl_max_lensing_step(cmbl_flow* L, int basis, const void* phi, const void* eta, int nb, double* out) {
  return guard([&] {
    NOTNULL(L); NOTNULL(phi); NOTNULL(eta); NOTNULL(out); BASIS_OK(basis); CMBL_REQUIRE(nb >= 1, ERR_SHAPE, "nbatch >= 1");
    L->p->max_lensing_step(basis, phi, eta, nb, out);
  });
}

// ---- small linear algebra / quadratic-estimate helpers ---------------------------------------------------
int cmbl_axpby(cmbl_ctx* ctx, int basis, const double* a, const void* x, const double* b, const void* y, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(a); NOTNULL(x); NOTNULL(out); BASIS_OK(basis); POLB_OK(P, B);
    CMBL_REQUIRE(y == nullptr || b != nullptr, ERR_ARG, "b is required when y is given");
    const long n = (basis == B_MAP ? ctx->p->npix() : 2 * ctx->p->plane()) * P;
    BY_DTYPE(ctx, do_axpby, ctx, a, x, b, y, out, n, B);
  });
}
int cmbl_qe_leg(cmbl_ctx* ctx, const void* in_fourier, int n, int p1, int p2, void* out_map, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(in_fourier); NOTNULL(out_map); CMBL_REQUIRE(B >= 1 && n >= 0 && p1 >= 0 && p2 >= 0, ERR_ARG, "bad leg indices");
    BY_DTYPE(ctx, do_qe_leg, ctx, in_fourier, n, p1, p2, out_map, B);
  });
}
int cmbl_fourier_lmul(cmbl_ctx* ctx, const void* in_map, int p1, int p2, int take_abs, void* out_fourier, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(in_map); NOTNULL(out_fourier); CMBL_REQUIRE(B >= 1 && p1 >= 0 && p2 >= 0, ERR_ARG, "bad exponents");
    BY_DTYPE(ctx, do_fourier_lmul, ctx, in_map, p1, p2, take_abs, out_fourier, B);
  });
}
int cmbl_map_fma(cmbl_ctx* ctx, const void* a, const void* b, double scale, void* out, int accumulate, int nslices) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(a); NOTNULL(b); NOTNULL(out); CMBL_REQUIRE(nslices >= 1, ERR_SHAPE, "nslices >= 1");
    const long n = ctx->p->npix() * nslices;
    BY_DTYPE(ctx, do_map_fma, ctx, a, b, scale, out, accumulate, n);
  });
}

int cmbl_randn(cmbl_ctx* ctx, const uint64_t* seeds, int nslots, uint64_t stream, void* out, long n_per_slot) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(seeds); NOTNULL(out);
    CMBL_REQUIRE(nslots >= 1 && n_per_slot >= 1, ERR_SHAPE, "nslots >= 1 and n_per_slot >= 1");
    BY_DTYPE(ctx, do_randn, ctx, seeds, nslots, stream, out, n_per_slot);
  });
}

// ---- dataset ---------------------------------------------------------------------------------------
int cmbl_dataset_create(cmbl_ctx* ctx, int npol, cmbl_dataset** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    auto h = std::make_unique<cmbl_dataset>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_dataset_create, h.get(), npol);
    registry_add(h.get());
    *out = h.release();
  });
}
int cmbl_dataset_destroy(cmbl_dataset* ds) { return guard([&] { if (ds) registry_remove(ds); delete ds; }); }
int cmbl_dataset_set_op(cmbl_dataset* ds, int which, const void* planes, int nplanes) {
  return guard([&] {
    NOTNULL(ds);
    if (!(which == CMBL_OP_CN_INV_PIX && nplanes == 0)) NOTNULL(planes);      // clearing the map-diagonal noise operator takes no planes
    ds->p->set_op(which, planes, nplanes);
  });
}
int cmbl_dataset_noise_inv(cmbl_dataset* ds, const void* in, void* out, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(in); NOTNULL(out); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    BY_DTYPE(ds->ctx, do_noise_inv, ds, in, out, B);
  });
}
int cmbl_dataset_set_data(cmbl_dataset* ds, const void* d, int B) {
  return guard([&] { NOTNULL(ds); NOTNULL(d); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1"); ds->p->set_data(d, B); });
}
int cmbl_dataset_set_logdet(cmbl_dataset* ds, double v) {
  return guard([&] { NOTNULL(ds); ds->p->logdet_sum = v; });
}

int cmbl_gradientf_logpdf(cmbl_dataset* ds, cmbl_flow* L, const void* f, const void* d, int zero_d, void* out, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(f); NOTNULL(out); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX(ds, L);
    cmbl_lensop v{L->ctx, LENSOP_FLOW, L};
    BY_DTYPE(ds->ctx, do_gradf_op, ds, &v, f, d, zero_d, out, B);
  });
}

int cmbl_wiener_cg(cmbl_dataset* ds, cmbl_flow* L, const void* d, const void* fstart, double tol, int maxit, void* f_out,
                   double* hist, int* nit, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(f_out); NOTNULL(hist); NOTNULL(nit);
    CMBL_REQUIRE(B >= 1 && maxit >= 1, ERR_ARG, "nbatch >= 1 and maxit >= 1");
    SAME_CTX(ds, L);
    cmbl_lensop v{L->ctx, LENSOP_FLOW, L};
    BY_DTYPE(ds->ctx, do_cg_op, ds, &v, d, fstart, tol, maxit, f_out, hist, nit, B);
  });
}

// ---- any lensing operator in the L slot: typed, non-owning views of the operator handles ----
int cmbl_lensop_from_lenseflow(cmbl_flow* L, cmbl_lensop** out) { return lensop_view(L, LENSOP_FLOW, out); }
int cmbl_lensop_from_bilinear(cmbl_bilinear* L, cmbl_lensop** out) { return lensop_view(L, LENSOP_BILINEAR, out); }
int cmbl_lensop_from_powerlens(cmbl_powerlens* L, cmbl_lensop** out) { return lensop_view(L, LENSOP_POWERLENS, out); }
int cmbl_lensop_identity(cmbl_ctx* ctx, cmbl_lensop** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    auto h = std::make_unique<cmbl_lensop>();
    h->ctx = ctx; h->kind = LENSOP_IDENTITY; h->h = nullptr;
    BY_DTYPE(ctx, do_lensop_identity, h.get());
    *out = h.release();
  });
}
int cmbl_lensop_destroy(cmbl_lensop* op) { return guard([&] { delete op; }); }

int cmbl_gradientf_logpdf_op(cmbl_dataset* ds, cmbl_lensop* L, const void* f, const void* d, int zero_d, void* out, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(f); NOTNULL(out); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX_OP(ds, L);
    BY_DTYPE(ds->ctx, do_gradf_op, ds, L, f, d, zero_d, out, B);
  });
}
int cmbl_wiener_cg_op(cmbl_dataset* ds, cmbl_lensop* L, const void* d, const void* fstart, double tol, int maxit, void* f_out,
                      double* hist, int* nit, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(f_out); NOTNULL(hist); NOTNULL(nit);
    CMBL_REQUIRE(B >= 1 && maxit >= 1, ERR_ARG, "nbatch >= 1 and maxit >= 1");
    SAME_CTX_OP(ds, L);
    BY_DTYPE(ds->ctx, do_cg_op, ds, L, d, fstart, tol, maxit, f_out, hist, nit, B);
  });
}
int cmbl_grad_logpdf_op(cmbl_dataset* ds, cmbl_lensop* L, const void* f, const void* phi, const void* d, double* lp, void* gf, void* gphi,
                        int B, int quirk) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(f); NOTNULL(phi); NOTNULL(lp); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX_OP(ds, L);
    BY_DTYPE(ds->ctx, do_grad_lp_op, ds, L, f, phi, d, lp, gf, gphi, B, quirk);
  });
}

int cmbl_nolensing_logpdf(cmbl_dataset* ds, const void* f, const void* d, double* lp_host, void* gf_out, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(f); NOTNULL(lp_host); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    BY_DTYPE(ds->ctx, do_nolens_logpdf, ds, f, d, lp_host, gf_out, B);
  });
}

int cmbl_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, double* lp, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(fo); NOTNULL(phio); NOTNULL(lp); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_lpm, ds, L, fo, phio, lp, nullptr, nullptr, B, 0);
  });
}
int cmbl_grad_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, double* lp, void* gfo, void* gphio, int B, int quirk) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(fo); NOTNULL(phio); NOTNULL(lp); NOTNULL(gfo); NOTNULL(gphio); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_lpm, ds, L, fo, phio, lp, gfo, gphio, B, quirk);
  });
}

// ---- θ layer: the parameter-dependent operators and logpdf(Mixed; θ) over a grid, on the device ----
int cmbl_dataset_theta_model(cmbl_dataset* ds, const double* Cfs_host, int nplanes, const double* C0_host, int nbands, const int* band_planes_host,
                             const int32_t* band_idx_host, const int* band_nbins_host, const double* Cten_host, const double* Cn_host, double s2len,
                             double r0, const double* Cphi0_host, double Aphi0, const double* Nphi_host, const double* G_host, double logdet_Cn) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(Cfs_host); NOTNULL(Cten_host); NOTNULL(Cn_host); NOTNULL(Cphi0_host); NOTNULL(Nphi_host);
    const ThetaModelArgs a{Cfs_host, nplanes, C0_host, nbands, band_planes_host, band_idx_host, band_nbins_host, Cten_host, Cn_host, s2len, r0,
                           Cphi0_host, Aphi0, Nphi_host, G_host, logdet_Cn};
    BY_DTYPE(ds->ctx, do_theta_model, ds, a);
  });
}
int cmbl_logpdf_mixed_theta(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, int B, int ntheta, const double* r_host,
                            const double* Aphi_host, const double* amps_host, int namps, double* lp_host) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(fo); NOTNULL(phio); NOTNULL(r_host); NOTNULL(Aphi_host); NOTNULL(lp_host);
    CMBL_REQUIRE(B >= 1 && ntheta >= 1, ERR_SHAPE, "nbatch >= 1 and ntheta >= 1");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_lpm_theta, ds, L, fo, phio, B, ntheta, r_host, Aphi_host, amps_host, namps, lp_host);
  });
}
int cmbl_dataset_theta_ops(cmbl_dataset* ds, double r, double Aphi, const double* amps_host, int namps, int which, void* out_dev, double* sums_host) {
  return guard([&] {
    NOTNULL(ds);
    BY_DTYPE(ds->ctx, do_theta_ops, ds, r, Aphi, amps_host, namps, which, out_dev, sums_host);
  });
}

int cmbl_grad_theta_logpdf(cmbl_dataset* ds, const void* f, const void* phi, int B, double r, double Aphi, const double* amps_host, int namps, int want,
                           double* grad_host) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(f); NOTNULL(phi); NOTNULL(grad_host); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    BY_DTYPE(ds->ctx, do_grad_theta, ds, f, phi, B, r, Aphi, amps_host, namps, want, grad_host);
  });
}
int cmbl_grad_theta_logpdf_mixed(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, int B, double r, double Aphi, const double* amps_host,
                                 int namps, int want, double* lp_host, double* grad_host) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(fo); NOTNULL(phio); NOTNULL(lp_host); NOTNULL(grad_host); CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_grad_theta_mixed, ds, L, fo, phio, B, r, Aphi, amps_host, namps, want, lp_host, grad_host);
  });
}

int cmbl_hmc_step(cmbl_dataset* ds, cmbl_flow* L, const void* fo, const void* phio, const void* mass, const void* white_p, const double* log_u_host,
                  const uint64_t* seeds_host, uint64_t step, int nleap, double eps, int always_accept, int alias_quirk, int B,
                  void* phio_out, double* dH_host, int* accept_host) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(fo); NOTNULL(phio); NOTNULL(mass); NOTNULL(phio_out); NOTNULL(dH_host); NOTNULL(accept_host);
    CMBL_REQUIRE(B >= 1 && B <= MAXBATCH && nleap >= 1, ERR_ARG, "1 <= nbatch <= 256 and nleap >= 1");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_hmc, ds, L, fo, phio, mass, white_p, log_u_host, seeds_host, step, nleap, eps, always_accept, alias_quirk, B, phio_out, dH_host, accept_host);
  });
}
int cmbl_map_joint_step(cmbl_dataset* ds, cmbl_flow* L, const void* phi, const void* fstart, const void* hinv, double alpha_max, double alpha_tol,
                        double cg_tol, int cg_maxit, int alias_quirk, int B, void* f_out, void* phi_out, double* logpdf_host, double* alpha_host,
                        int* ncg_host, int* nls_host) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(L); NOTNULL(phi); NOTNULL(hinv); NOTNULL(f_out); NOTNULL(phi_out); NOTNULL(logpdf_host); NOTNULL(alpha_host); NOTNULL(ncg_host); NOTNULL(nls_host);
    CMBL_REQUIRE(B >= 1 && B <= MAXBATCH && cg_maxit >= 1 && alpha_max > 0 && alpha_tol > 0, ERR_ARG, "1 <= nbatch <= 256, cg_maxit >= 1, alpha_max > 0, alpha_tol > 0");
    SAME_CTX(ds, L);
    BY_DTYPE(ds->ctx, do_map_step, ds, L, phi, fstart, hinv, alpha_max, alpha_tol, cg_tol, cg_maxit, alias_quirk, B, f_out, phi_out, logpdf_host, alpha_host, ncg_host, nls_host);
  });
}

int cmbl_quadratic_estimate(cmbl_dataset* ds, int which, const double* Cf_host, const double* Cftilde_host, const double* Cn_host, const double* TF_host,
                            const double* Cphi_host, int wiener_filtered, const double* AL_in_host, void* phiqe_out, double* AL_out_host, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(Cf_host); NOTNULL(Cftilde_host); NOTNULL(Cn_host); NOTNULL(TF_host); NOTNULL(Cphi_host); NOTNULL(phiqe_out);
    CMBL_REQUIRE(which >= 0 && which <= 2, ERR_ARG, "which: 0 = TT, 1 = EE, 2 = EB (src/quadratic_estimate.jl:41: the others are not implemented by the reference either)");
    CMBL_REQUIRE(B >= 1, ERR_SHAPE, "nbatch >= 1");
    BY_DTYPE(ds->ctx, do_qe, ds, which, Cf_host, Cftilde_host, Cn_host, TF_host, Cphi_host, wiener_filtered, AL_in_host, phiqe_out, AL_out_host, B);
  });
}

// ---- ud_grade: the one entry point with two contexts ---------------------------------------------------------------
int cmbl_ud_grade(cmbl_ctx* src, cmbl_ctx* dst, int mode, int deconv_pixwin, int anti_aliasing, int bi, const void* in, int bo, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(src); NOTNULL(dst); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    const CtxBase& s = *src->p; const CtxBase& d = *dst->p;
    CMBL_REQUIRE(s.dtype == d.dtype && s.device == d.device && s.stream == d.stream, ERR_ARG, "ud_grade: the two contexts must share dtype, device and stream");
    CMBL_REQUIRE(mode == CMBL_UD_MAP || mode == CMBL_UD_FOURIER, ERR_ARG, "mode must be CMBL_UD_MAP or CMBL_UD_FOURIER");
    CMBL_REQUIRE((bi == B_HARMONIC) == (bo == B_HARMONIC), ERR_ARG, "ud_grade: HARMONIC is accepted on both sides at once only (the engine has no EB-map basis)");
    CMBL_REQUIRE(bi != B_HARMONIC || mode == CMBL_UD_FOURIER, ERR_ARG, "ud_grade: HARMONIC planes are accepted in Fourier mode only");
    const size_t el = s.dtype == CMBL_F32 ? 4 : 8, sl = (size_t)P * B;
    const char* a = (const char*)in; const char* b = (const char*)out;
    const size_t na = sl * el * (bi == B_MAP ? (size_t)s.npix() : 2 * (size_t)s.plane()), nb = sl * el * (bo == B_MAP ? (size_t)d.npix() : 2 * (size_t)d.plane());
    CMBL_REQUIRE(a + na <= b || b + nb <= a, ERR_ARG, "ud_grade: in and out must not alias");
    BY_DTYPE(src, do_ud_grade, src, dst, mode, deconv_pixwin, anti_aliasing, bi, in, bo, out, P, B);
  });
}
int cmbl_pixwin_host(cmbl_ctx* ctx, double* out_host, size_t n) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out_host);
    CMBL_REQUIRE(n == (size_t)ctx->p->plane(), ERR_SHAPE, "pixwin output has the wrong length");
    pixwin_plane(*ctx->p, out_host);
  });
}

// ---- get_Cℓ: the binning plan (host, double) and the binned sums on the device -----------------------------------------
int cmbl_clbins_create(cmbl_ctx* ctx, const double* ledges_host, int nedges, const double* w_host, size_t nw, cmbl_clbins** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(ledges_host); NOTNULL(out);
    CMBL_REQUIRE(nedges >= 2 && nedges <= 65536, ERR_ARG, "clbins: 2 <= nedges <= 65536");
    for (int i = 0; i < nedges; ++i) CMBL_REQUIRE(std::isfinite(ledges_host[i]) && (i == 0 || ledges_host[i] > ledges_host[i - 1]), ERR_ARG, "clbins: the edges must be finite and strictly increasing");
    if (w_host) {
      CMBL_REQUIRE(nw == (size_t)ctx->p->plane(), ERR_SHAPE, "clbins: the weight plane has the wrong length");
      for (size_t i = 0; i < nw; ++i) CMBL_REQUIRE(std::isfinite(w_host[i]), ERR_ARG, "clbins: the weights must be finite (apply nan2zero first)");
    }
    auto h = std::make_unique<cmbl_clbins>();
    h->p = std::make_unique<ClBins>(*ctx->p, ledges_host, nedges, w_host);
    *out = h.release();
  });
}
int cmbl_clbins_destroy(cmbl_clbins* bins) { return guard([&] { delete bins; }); }
int cmbl_clbins_info_host(cmbl_clbins* bins, int which, double* out_host, size_t n) {
  return guard([&] {
    NOTNULL(bins); NOTNULL(out_host);
    const ClBins& b = *bins->p;
    const std::vector<double>* v = which == CMBL_CL_A ? &b.A : which == CMBL_CL_SL ? &b.Sl : which == CMBL_CL_COUNT ? &b.count : nullptr;
    CMBL_REQUIRE(v != nullptr, ERR_ARG, "clbins: bad selector");
    CMBL_REQUIRE(n == v->size(), ERR_SHAPE, "clbins: output has the wrong length (nedges - 1)");
    std::memcpy(out_host, v->data(), n * sizeof(double));
  });
}
int cmbl_get_cl(cmbl_ctx* ctx, cmbl_clbins* bins, int basis, const void* f1, const void* f2, int P, int B, const int* pairs_host, int npairs, int moments, double* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(bins); NOTNULL(f1); NOTNULL(pairs_host); NOTNULL(out); BASIS_OK(basis); POLB_OK(P, B);
    CMBL_REQUIRE(B <= MAXBATCH, ERR_ARG, "nbatch > 256 not supported in reductions");
    CMBL_REQUIRE(npairs >= 1 && npairs <= CL_MAXPAIRS, ERR_ARG, "get_cl: 1 <= npairs <= 9");
    CMBL_REQUIRE(moments == 1 || moments == 2, ERR_ARG, "get_cl: moments must be 1 (S1) or 2 (S1, S2)");
    ClPairs pr{};
    pr.n = npairs;
    for (int k = 0; k < npairs; ++k) {
      const int a = pairs_host[2 * k], b = pairs_host[2 * k + 1];
      CMBL_REQUIRE(a >= 0 && a < P && b >= 0 && b < P, ERR_ARG, "get_cl: a pair indexes a plane outside [0, npol)");
      pr.a[k] = (signed char)a; pr.b[k] = (signed char)b;
    }
    BY_DTYPE(ctx, do_get_cl, ctx, bins, basis, f1, f2, P, B, pr, moments, out);
  });
}

// ---- BilinearLens (src/bilinearlens.jl) ------------------------------------------------------------------------------
int cmbl_bilinear_create(cmbl_ctx* ctx, cmbl_bilinear** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    auto h = std::make_unique<cmbl_bilinear>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_bl_create, h.get());
    *out = h.release();
  });
}
int cmbl_bilinear_destroy(cmbl_bilinear* L) { return guard([&] { delete L; }); }
int cmbl_bilinear_set_phi(cmbl_bilinear* L, int basis, const void* phi, int nb) {
  return guard([&] {
    NOTNULL(L); NOTNULL(phi); BASIS_OK(basis); CMBL_REQUIRE(nb >= 1, ERR_SHAPE, "nbatch_phi >= 1");
    L->p->set_phi(basis, phi, nb);
  });
}
int cmbl_bilinear_set_deflection(cmbl_bilinear* L, const void* dy_px, const void* dx_px) {
  return guard([&] {
    NOTNULL(L); NOTNULL(dy_px); NOTNULL(dx_px);
    L->p->set_deflection(dy_px, dx_px);
  });
}
int cmbl_bilinear_apply(cmbl_bilinear* L, int mode, int bi, const void* in, int bo, void* out, int P, int B, int maxiter) {
  return guard([&] {
    NOTNULL(L); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    CMBL_REQUIRE(mode >= 0 && mode <= 3, ERR_ARG, "bad flow mode");
    CMBL_REQUIRE(maxiter >= 1 && maxiter <= BL_MAXIT, ERR_ARG, "maxiter must lie in [1, 16]");
    L->p->apply(mode, bi, in, bo, out, P, B, maxiter);
  });
}
int cmbl_bilinear_grad(cmbl_bilinear* L, const void* f_lensed, int bdel, const void* delta, void* dphi, int bdf, void* df, int P, int B) {
  return guard([&] {
    NOTNULL(L); NOTNULL(f_lensed); NOTNULL(delta); NOTNULL(dphi); NOTNULL(df); BASIS_OK(bdel); BASIS_OK(bdf); POLB_OK(P, B);
    L->p->grad(f_lensed, bdel, delta, dphi, bdf, df, P, B);
  });
}

// ---- PowerLens / Taylens (src/powerlens.jl, src/taylens.jl) ------------------------------------------------------------
int cmbl_powerlens_create(cmbl_ctx* ctx, int order, int kind, cmbl_powerlens** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    CMBL_REQUIRE(order >= 0 && order <= PL_MAXORDER, ERR_ARG, "order must lie in [0, 12] (PowerLens(phi, order), src/powerlens.jl:22-29)");
    CMBL_REQUIRE(kind == CMBL_POWERLENS || kind == CMBL_TAYLENS, ERR_ARG, "kind must be CMBL_POWERLENS (src/powerlens.jl) or CMBL_TAYLENS (src/taylens.jl)");
    auto h = std::make_unique<cmbl_powerlens>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_pl_create, h.get(), order, kind);
    *out = h.release();
  });
}
int cmbl_powerlens_destroy(cmbl_powerlens* L) { return guard([&] { delete L; }); }
int cmbl_powerlens_set_phi(cmbl_powerlens* L, int basis, const void* phi, int nb) {
  return guard([&] {
    NOTNULL(L); NOTNULL(phi); BASIS_OK(basis);
    L->p->set_phi(basis, phi, nb);
  });
}
int cmbl_powerlens_set_deflection(cmbl_powerlens* L, const void* dy_rad, const void* dx_rad) {
  return guard([&] {
    NOTNULL(L); NOTNULL(dy_rad); NOTNULL(dx_rad);
    L->p->set_deflection(dy_rad, dx_rad);
  });
}
int cmbl_powerlens_apply(cmbl_powerlens* L, int mode, int bi, const void* in, int bo, void* out, int P, int B) {
  return guard([&] {
    NOTNULL(L); NOTNULL(in); NOTNULL(out); BASIS_OK(bi); BASIS_OK(bo); POLB_OK(P, B);
    CMBL_REQUIRE(mode >= 0 && mode <= 3, ERR_ARG, "bad flow mode");
    L->p->apply(mode, bi, in, bo, out, P, B);
  });
}

// ---- make_mask (src/masking.jl:1-67) -------------------------------------------------------------------------------------
int cmbl_edt_sq(cmbl_ctx* ctx, const uint8_t* feat_dev, int32_t* d2_dev) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(feat_dev); NOTNULL(d2_dev);
    BY_DTYPE(ctx, do_edt_sq, ctx, feat_dev, d2_dev);
  });
}
int cmbl_make_mask(cmbl_ctx* ctx, const int32_t* src_yx_host, int nsrc, int pad, int apod_w, int round_w, int src_w, void* out_map_dev) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out_map_dev);
    const CtxBase& c = *ctx->p;
    CMBL_REQUIRE(nsrc >= 0 && pad >= 0 && apod_w >= 0 && round_w >= 0 && src_w >= 0, ERR_ARG, "make_mask: the source count and the widths must not be negative");
    CMBL_REQUIRE(apod_w == 0 || pad > 0, ERR_ARG, "make_mask: apodisation needs edge padding (without it there is no masked pixel to measure the distance to)");
    CMBL_REQUIRE(nsrc == 0 || src_w > 0, ERR_ARG, "make_mask: point sources need a radius of at least one pixel");
    CMBL_REQUIRE(nsrc == 0 || src_yx_host != nullptr, ERR_ARG, "make_mask: nsrc > 0 needs src_yx_host");
    CMBL_REQUIRE(round_w <= MASK_MAXSIGMA, ERR_ARG, "make_mask: round_w must not exceed 1024 pixels");
    CMBL_REQUIRE(pad <= EDT_MAXN && apod_w <= (1 << 20) && src_w <= 2 * EDT_MAXN, ERR_ARG, "make_mask: a width far beyond the largest map");
    for (int s = 0; s < nsrc; ++s)
      CMBL_REQUIRE(src_yx_host[2 * s] >= 0 && src_yx_host[2 * s] < c.Ny && src_yx_host[2 * s + 1] >= 0 && src_yx_host[2 * s + 1] < c.Nx, ERR_ARG, "make_mask: a point source lies outside the map");
    const MaskArgs m{src_yx_host, nsrc, pad, apod_w, round_w, src_w};
    BY_DTYPE(ctx, do_make_mask, ctx, m, out_map_dev);
  });
}

// ---- ProjEquiRect (src/proj_equirect.jl) -----------------------------------------------------------------------------------
// ProjEquiRect(; Ny, Nx, θspan, φspan) (:71-81, 112-120): host, double, no context
int cmbl_equirect_geometry_host(int Ny, int Nx, const double* theta_span, const double* phi_span, double* theta, double* phi,
                                double* theta_edges, double* phi_edges, double* omega, double* lx) {
  return guard([&] {
    NOTNULL(theta_span); NOTNULL(phi_span);
    CMBL_REQUIRE(Ny >= 2 && Nx >= 2 && Ny <= 4096 && Nx <= 4096, ERR_SHAPE, "Ny and Nx must lie in [2, 4096]");
    CMBL_REQUIRE(theta_span[0] != theta_span[1] && phi_span[0] != phi_span[1], ERR_ARG, "equirect_geometry: an empty span");
    equirect_geometry(Ny, Nx, theta_span, phi_span, theta, phi, theta_edges, phi_edges, omega, lx);
  });
}
// AzFourier / Map (:149-157), QUAzFourier / QUMap (:160-178)
int cmbl_equirect_convert(cmbl_ctx* ctx, int bi, const void* in, int bo, void* out, int npol, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(in); NOTNULL(out);
    CMBL_REQUIRE((bi == CMBL_MAP || bi == CMBL_AZFOURIER) && (bo == CMBL_MAP || bo == CMBL_AZFOURIER), ERR_ARG, "equirect_convert: the bases are CMBL_MAP and CMBL_AZFOURIER");
    CMBL_REQUIRE(npol == 1 || npol == 2, ERR_ARG, "equirect_convert: npol must be 1 or 2 (IQUAzFourier has no transform in the reference)");
    CMBL_REQUIRE(B >= 1 && B <= 65535, ERR_SHAPE, "equirect_convert: nbatch must lie in [1, 65535]");
    CMBL_REQUIRE(npol == 1 || ctx->p->Nx % 2 == 0, ERR_SHAPE, "equirect_convert: QUAzFourier needs an even Nx (src/proj_equirect.jl:166 is a dimension mismatch otherwise)");
    CMBL_REQUIRE(in != out, ERR_ARG, "equirect_convert: in and out must not be the same array");
    BY_DTYPE(ctx, do_eq_convert, ctx, bi, in, bo, out, npol, B);
  });
}
#define EQ_N_OK(ctx, n) CMBL_REQUIRE((n) == (ctx)->p->Ny || (n) == 2 * (ctx)->p->Ny, ERR_SHAPE, "equirect: n must be Ny or 2 Ny")
// M * f, M' * f (:230-240)
int cmbl_equirect_block_apply(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, int adjoint, const void* in, void* out, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(blocks); NOTNULL(in); NOTNULL(out);
    EQ_N_OK(ctx, n);
    CMBL_REQUIRE(B >= 1, ERR_SHAPE, "equirect_block_apply: nbatch >= 1");
    CMBL_REQUIRE(in != out && blocks != out, ERR_ARG, "equirect_block_apply: out must not alias an input");
    BY_DTYPE(ctx, do_eq_apply, ctx, blocks, blocks_complex != 0, n, adjoint != 0, in, out, B);
  });
}
// M1 * M2, M1' * M2, M1 * M2' (:254-269)
int cmbl_equirect_block_matmul(cmbl_ctx* ctx, const void* A, int adjA, const void* B, int adjB, int blocks_complex, int n, void* out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(A); NOTNULL(B); NOTNULL(out);
    EQ_N_OK(ctx, n);
    CMBL_REQUIRE(!(adjA && adjB), ERR_ARG, "equirect_block_matmul: the reference has no product of two adjoints");
    CMBL_REQUIRE(out != A && out != B, ERR_ARG, "equirect_block_matmul: out must not alias an input");
    BY_DTYPE(ctx, do_eq_matmul, ctx, A, adjA != 0, B, adjB != 0, blocks_complex != 0, n, out);
  });
}
// dot(M1', M2) (:358-360)
int cmbl_equirect_block_dot(cmbl_ctx* ctx, const void* A, const void* B, int blocks_complex, int n, double* out_host) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(A); NOTNULL(B); NOTNULL(out_host);
    EQ_N_OK(ctx, n);
    BY_DTYPE(ctx, do_eq_dot, ctx, A, B, blocks_complex != 0, n, out_host);
  });
}
// Cℓ_to_Beam(:I) (:505-515): blocks[j, k, m] *= w[k]
int cmbl_equirect_block_scale_columns(cmbl_ctx* ctx, void* blocks, int blocks_complex, int n, const double* w_host, int nw) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(blocks); NOTNULL(w_host);
    EQ_N_OK(ctx, n);
    CMBL_REQUIRE(nw == n, ERR_SHAPE, "equirect_block_scale_columns: one weight per column");
    BY_DTYPE(ctx, do_eq_scale_columns, ctx, blocks, blocks_complex != 0, n, w_host);
  });
}
// Cℓ_to_Beam(:P) (:517-533): [B 0; 0 B] * diag(Ω, Ω)
int cmbl_equirect_beam_pol(cmbl_ctx* ctx, const void* blocksI_real, const double* omega_host, void* out_complex) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(blocksI_real); NOTNULL(omega_host); NOTNULL(out_complex);
    CMBL_REQUIRE(blocksI_real != out_complex, ERR_ARG, "equirect_beam_pol: out must not alias the input");
    BY_DTYPE(ctx, do_eq_beam_pol, ctx, blocksI_real, omega_host, out_complex);
  });
}
// Cℓ_to_Cov(:I / :P) (:430-503): the covariance of the AzFourier / QUAzFourier coefficients of an isotropic field, in double, rounded at the store
int cmbl_equirect_cov(cmbl_ctx* ctx, const double* theta_span, const double* phi_span, int pol, int lmax, const double* cl_a, const double* cl_b,
                      int ngrid, void* blocks_out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(theta_span); NOTNULL(phi_span); NOTNULL(cl_a); NOTNULL(blocks_out);
    CMBL_REQUIRE(pol == 0 || pol == 2, ERR_ARG, "equirect_cov: pol is 0 (I) or 2 (P)");
    CMBL_REQUIRE(pol == 0 || cl_b != nullptr, ERR_ARG, "equirect_cov: P needs the EE and the BB spectrum");
    CMBL_REQUIRE(theta_span[0] != theta_span[1] && phi_span[0] != phi_span[1], ERR_ARG, "equirect_cov: an empty span");
    CMBL_REQUIRE(equirect_span_K(phi_span) >= 1, ERR_SHAPE, "equirect_cov: the azimuthal span must be 2 pi / K for an integer K (no block-diagonal covariance otherwise)");
    CMBL_REQUIRE(pol == 0 || ctx->p->Nx % 2 == 0, ERR_SHAPE, "equirect_cov: QUAzFourier needs an even Nx");
    CMBL_REQUIRE(lmax >= (pol == 0 ? 0 : 2) && lmax <= 100000, ERR_SHAPE, "equirect_cov: lmax must be at least 0 (I) or 2 (P) and at most 100000 (the integer recurrence coefficients stay exact in double)");
    CMBL_REQUIRE(ngrid == 0 || (ngrid >= 4 && ngrid <= (1 << 24)), ERR_SHAPE, "equirect_cov: ngrid is 0 (exact mode) or at least 4 (the interpolation stencil)");
    for (int l = 0; l <= lmax; ++l)
      CMBL_REQUIRE(std::isfinite(cl_a[l]) && (pol == 0 || std::isfinite(cl_b[l])), ERR_NAN, "equirect_cov: a spectrum value is not finite");
    BY_DTYPE(ctx, do_eq_cov, ctx, theta_span, phi_span, pol, lmax, cl_a, cl_b, ngrid, blocks_out);
  });
}
// sqrt / pinv / singular values (:313-323), log|det| (:342-347) and the solves (:274-282) of the blocks, factorised on the device in double
#define EQ_FACTOR_N_OK(n) CMBL_REQUIRE((n) <= 2048, ERR_SHAPE, "equirect: the device factorisations take blocks of n <= 2048")
int cmbl_equirect_block_svd(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, double rtol, void* out_sqrt, void* out_pinv, double* sv_host, int* sweeps_host) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(blocks);
    EQ_N_OK(ctx, n); EQ_FACTOR_N_OK(n);
    CMBL_REQUIRE(rtol >= 0.0 && std::isfinite(rtol), ERR_ARG, "equirect_block_svd: rtol must be finite and not negative");
    CMBL_REQUIRE(out_sqrt != blocks && out_pinv != blocks && (out_sqrt == nullptr || out_sqrt != out_pinv), ERR_ARG, "equirect_block_svd: an output must not alias the input or the other output");
    BY_DTYPE(ctx, do_eq_svd, ctx, blocks, blocks_complex != 0, n, rtol, out_sqrt, out_pinv, sv_host, sweeps_host);
  });
}
int cmbl_equirect_block_logabsdet(cmbl_ctx* ctx, const void* blocks, int blocks_complex, int n, double* out_host) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(blocks); NOTNULL(out_host);
    EQ_N_OK(ctx, n); EQ_FACTOR_N_OK(n);
    BY_DTYPE(ctx, do_eq_logabsdet, ctx, blocks, blocks_complex != 0, n, out_host);
  });
}
int cmbl_equirect_block_solve(cmbl_ctx* ctx, const void* A, int a_complex, int n, int side, const void* rhs, int rhs_complex, int rhs_kind, void* out, int B) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(A); NOTNULL(rhs); NOTNULL(out);
    EQ_N_OK(ctx, n); EQ_FACTOR_N_OK(n);
    CMBL_REQUIRE(side == CMBL_SIDE_LEFT || side == CMBL_SIDE_RIGHT, ERR_ARG, "equirect_block_solve: side is CMBL_SIDE_LEFT or CMBL_SIDE_RIGHT");
    CMBL_REQUIRE(rhs_kind == CMBL_RHS_BLOCKS || rhs_kind == CMBL_RHS_FIELD, ERR_ARG, "equirect_block_solve: rhs_kind is CMBL_RHS_BLOCKS or CMBL_RHS_FIELD");
    CMBL_REQUIRE(rhs_kind == CMBL_RHS_BLOCKS || (side == CMBL_SIDE_LEFT && rhs_complex != 0), ERR_ARG, "equirect_block_solve: a field is complex and is solved from the left");
    CMBL_REQUIRE(rhs_kind == CMBL_RHS_BLOCKS || (B >= 1 && B <= 65535), ERR_SHAPE, "equirect_block_solve: nbatch must lie in [1, 65535]");
    CMBL_REQUIRE(out != A && out != rhs, ERR_ARG, "equirect_block_solve: out must not alias an input");
    BY_DTYPE(ctx, do_eq_solve, ctx, A, a_complex != 0, n, side, rhs, rhs_complex != 0, rhs_kind, out, B);
  });
}

// ---- NoLensingDataSet on ProjEquiRect (engine_equirect_ds.hpp) ---------------------------------------------------------------
int cmbl_eqds_create(cmbl_ctx* ctx, int npol, cmbl_eqds** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(out);
    auto h = std::make_unique<cmbl_eqds>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_eqds_create, h.get(), npol);
    *out = h.release();
  });
}
int cmbl_eqds_destroy(cmbl_eqds* ds) { return guard([&] { delete ds; }); }
int cmbl_eqds_set_block_op(cmbl_eqds* ds, int which, const void* blocks_dev, int blocks_complex, int n) {
  return guard([&] { NOTNULL(ds); ds->p->set_block_op(which, blocks_dev, blocks_complex != 0, n); });
}
int cmbl_eqds_set_pixel_op(cmbl_eqds* ds, int which, const void* map_dev, int nplanes) {
  return guard([&] { NOTNULL(ds); ds->p->set_pixel_op(which, map_dev, nplanes); });
}
int cmbl_eqds_set_logdet(cmbl_eqds* ds, double v) { return guard([&] { NOTNULL(ds); ds->p->logdet_sum = v; }); }
int cmbl_eqds_mean(cmbl_eqds* ds, const void* f, void* d_out, int B) {
  return guard([&] { NOTNULL(ds); NOTNULL(f); NOTNULL(d_out); ds->p->mean(f, d_out, B); });
}
int cmbl_eqds_gradientf_logpdf(cmbl_eqds* ds, const void* f, const void* d, void* out, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(out);
    CMBL_REQUIRE(out != f, ERR_ARG, "eqds_gradientf_logpdf: out must not alias f");
    ds->p->gradientf(f, d, out, B);
  });
}
int cmbl_eqds_logpdf(cmbl_eqds* ds, const void* f, const void* d, double* lp, int B) {
  return guard([&] { NOTNULL(ds); NOTNULL(f); NOTNULL(d); NOTNULL(lp); ds->p->logpdf(f, d, lp, B); });
}
int cmbl_eqds_wiener_cg(cmbl_eqds* ds, const void* d, const void* fstart, double tol, int maxit, void* f_out, double* hist, int* nit, int B) {
  return guard([&] {
    NOTNULL(ds); NOTNULL(d); NOTNULL(f_out); NOTNULL(hist); NOTNULL(nit);
    CMBL_REQUIRE(maxit >= 1, ERR_ARG, "eqds_wiener_cg: maxit >= 1");
    *nit = ds->p->wiener_cg(d, fstart, tol, maxit, f_out, hist, B);
  });
}
int cmbl_equirect_field_dot(cmbl_ctx* ctx, int basis, const void* a, const void* b, int npol, int B, double* out_host) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(a); NOTNULL(b); NOTNULL(out_host);
    CMBL_REQUIRE(basis == CMBL_MAP || basis == CMBL_AZFOURIER, ERR_ARG, "equirect_field_dot: the bases are CMBL_MAP and CMBL_AZFOURIER");
    CMBL_REQUIRE(npol == 1 || npol == 2, ERR_ARG, "equirect_field_dot: npol must be 1 or 2");
    CMBL_REQUIRE(npol == 1 || ctx->p->Nx % 2 == 0, ERR_SHAPE, "equirect_field_dot: QUAzFourier needs an even Nx");
    CMBL_REQUIRE(B >= 1 && B <= 65535, ERR_SHAPE, "equirect_field_dot: nbatch must lie in [1, 65535]");
    BY_DTYPE(ctx, do_eq_field_dot, ctx, basis, a, b, npol, B, out_host);
  });
}

// ---- HEALPix <-> Cartesian projection (src/proj_healpix.jl) ------------------------------------------------------------------
int cmbl_healpix_pix2ang_host(int nside, long first, long n, double* theta, double* phi) {
  return guard([&] {
    NOTNULL(theta); NOTNULL(phi);
    CMBL_REQUIRE(hpx_nside_ok(nside), ERR_SHAPE, "Nside must be a power of two in 1 ... 8192");
    CMBL_REQUIRE(first >= 0 && n >= 0 && first + n <= 12L * nside * nside, ERR_ARG, "pix2ang: pixel range outside [0, 12 Nside^2)");
    for (long k = 0; k < n; ++k) hpx_pix2ang(nside, first + k, theta + k, phi + k);
  });
}
int cmbl_projector_create(cmbl_ctx* ctx, int nside, int cart_kind, const double* params, cmbl_projector** out) {
  return cmbl_projector_create_method(ctx, nside, cart_kind, params, CMBL_PROJECT_BILINEAR, out);
}
int cmbl_projector_create_method(cmbl_ctx* ctx, int nside, int cart_kind, const double* params, int method, cmbl_projector** out) {
  return guard([&] {
    NOTNULL(ctx); NOTNULL(params); NOTNULL(out);
    CMBL_REQUIRE(method == CMBL_PROJECT_BILINEAR || method == CMBL_PROJECT_NFFT, ERR_ARG, "method must be CMBL_PROJECT_BILINEAR or CMBL_PROJECT_NFFT");
    CMBL_REQUIRE(hpx_nside_ok(nside), ERR_SHAPE, "Nside must be a power of two in 1 ... 8192");
    CMBL_REQUIRE(cart_kind == CMBL_PROJ_LAMBERT || cart_kind == CMBL_PROJ_EQUIRECT, ERR_ARG, "cart_kind must be CMBL_PROJ_LAMBERT or CMBL_PROJ_EQUIRECT");
    for (int k = 0; k < (cart_kind == CMBL_PROJ_LAMBERT ? 3 : 4); ++k) CMBL_REQUIRE(std::isfinite(params[k]), ERR_ARG, "projector: params must be finite");
    auto h = std::make_unique<cmbl_projector>();
    h->ctx = ctx;
    BY_DTYPE(ctx, do_projector_create, h.get(), nside, cart_kind, params, method);
    *out = h.release();
  });
}
int cmbl_projector_destroy(cmbl_projector* P) { return guard([&] { delete P; }); }
int cmbl_projector_method(cmbl_projector* P, int* method, int* window_width) {
  return guard([&] { NOTNULL(P); NOTNULL(method); NOTNULL(window_width); *method = P->p->method(); *window_width = P->p->width(); });
}
int cmbl_projector_info_host(cmbl_projector* P, int which, double* out_host, size_t n) {
  return guard([&] { NOTNULL(P); NOTNULL(out_host); P->p->info(which, out_host, n); });
}
int cmbl_project_to_cart(cmbl_projector* P, const void* hpx, void* map_out, int npol, int nbatch) {
  return guard([&] {
    NOTNULL(P); NOTNULL(hpx); NOTNULL(map_out); POLB_OK(npol, nbatch);
    CMBL_REQUIRE(hpx != map_out, ERR_ARG, "project_to_cart: out must not alias the input");
    P->p->to_cart(hpx, map_out, npol, nbatch);
  });
}
int cmbl_project_to_healpix(cmbl_projector* P, int basis_in, const void* in, void* hpx_out, int npol, int nbatch) {
  return guard([&] {
    NOTNULL(P); NOTNULL(in); NOTNULL(hpx_out); BASIS_OK(basis_in); POLB_OK(npol, nbatch);
    CMBL_REQUIRE(in != hpx_out, ERR_ARG, "project_to_healpix: out must not alias the input");
    P->p->to_healpix(basis_in, in, hpx_out, npol, nbatch);
  });
}
int cmbl_project_to_cart_adjoint(cmbl_projector* P, const void* map_cot, void* hpx_out, int npol, int nbatch) {
  return guard([&] {
    NOTNULL(P); NOTNULL(map_cot); NOTNULL(hpx_out); POLB_OK(npol, nbatch);
    CMBL_REQUIRE(map_cot != hpx_out, ERR_ARG, "project_to_cart_adjoint: out must not alias the input");
    P->p->to_cart_adjoint(map_cot, hpx_out, npol, nbatch);
  });
}
int cmbl_project_to_healpix_adjoint(cmbl_projector* P, const void* hpx_cot, void* map_out, int npol, int nbatch) {
  return guard([&] {
    NOTNULL(P); NOTNULL(hpx_cot); NOTNULL(map_out); POLB_OK(npol, nbatch);
    CMBL_REQUIRE(hpx_cot != map_out, ERR_ARG, "project_to_healpix_adjoint: out must not alias the input");
    P->p->to_healpix_adjoint(hpx_cot, map_out, npol, nbatch);
  });
}

#ifdef CMBL_STAMPS
// phase timestamps of the last stamped launch (tools/gpu_stamps*.py) of the translation unit CMBL_STAMPS_TU (kernels_fft.hpp CMBL_STAMPS_READER)
int cmbl_debug_stamps(unsigned long long* out_host, int n) {
  return guard([&] {
    CMBL_HIP(hipDeviceSynchronize());
    const char* e = std::getenv("CMBL_STAMPS_TU");
    const std::string u = e ? e : "main_f32";
    int rc = -1;
#define CMBL_X(unit) if (u == #unit) rc = cmbl::stamps_read_##unit(out_host, n);
    CMBL_STAMPS_UNITS(CMBL_X)
#undef CMBL_X
    CMBL_REQUIRE(rc == 0, ERR_ARG, "CMBL_STAMPS_TU: main_{f32,f64} | gen_{f32,f64} | small_{f32,f64} | cty_{f32,f64}_{a,b} | ctx_{f32,f64}_{a,b}");
  });
}
#endif

}  // extern "C"
