"""NumPy restatement of the reference's NoLensingDataSet (src/dataset.jl:37-47, 59-80, 129-132) and of argmaxf_logpdf (src/maximization.jl:17-42) on
ProjEquiRect, composed from tests/_equirect_ref.py (bases, block products) and oracle/cg.py (the reference's conjugate_gradient):

    d = M B f + noise,  f ~ N(0, Cf),  noise ~ N(0, Cn)

with Cf, B (and Cn in its block form) BlockDiagEquiRect blocks [m, q, p], M (and Cn in its pixel form, a VARIANCE map) map-diagonal planes
(P or 1, Nx, Ny).  The reference's argmaxf_logpdf begins with zero(diag(ds.Cf)) and defines no diag(::BlockDiagEquiRect), so it has no number to compare
with: this is its algorithm on its operators with the zero field of Cf's basis.  `wiener` holds the CG vectors as MAPS and uses the map dot, the
reference's bases; `wiener_az` holds them in the Az basis with the weighted dot the device uses -- the two agree only when every block operator maps
images of maps to images of maps (tests/test_equirect_ds_ref.py).

Every function computes in `dt` (np.float32 or np.float64): the float32 run against the float64 run on the same inputs is the budget of the GPU
tests (tools/make_equirect_dataset_budget.py).  Inputs are float32-representable."""
import numpy as np

import _equirect_ref as R
from oracle.cg import conjugate_gradient

# (Ny, Nx, nbatch, spin, form): form "pix": mask, B, Cn a variance map; "blk": mask, B, Cn block-diagonal; "bare": no B, no M, Cn a variance map
CASES = [(17, 30, 3, 0, "pix"), (17, 30, 3, 2, "pix"), (33, 45, 1, 0, "pix"), (96, 64, 3, 0, "pix"), (96, 64, 3, 2, "pix"), (32, 64, 9, 0, "pix"),
         (17, 30, 3, 0, "blk"), (17, 30, 3, 2, "blk"), (17, 30, 3, 0, "bare"), (17, 30, 3, 2, "bare")]
NSTEPS = 8


def case_id(c):
    return f"{c[0]}x{c[1]}_B{c[2]}_s{c[3]}_{c[4]}"


def _r32(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.real.astype(np.float32).astype(np.float64) + 1j * a.imag.astype(np.float32).astype(np.float64)
    return a.astype(np.float32).astype(np.float64)


def swap_conj(H):
    """S conj(H) S for blocks [m, q, p] of size 2 Ny: S swaps the two halves"""
    h = H.shape[-1] // 2
    return np.conj(np.roll(H, h, axis=(-2, -1)))


def symmetrise(H, Nx, spin2):
    """make the blocks at columns 0 and Nx/2 map images of maps to images of maps: real (spin 0), H <- (H + S conj(H) S) / 2 (spin 2)"""
    H = np.array(H)
    for m in ([0, Nx // 2] if Nx % 2 == 0 else [0]):
        H[m] = 0.5 * (H[m] + swap_conj(H[m])) if spin2 else H[m].real
    return H


def sym_spd_blocks(n, Mh, cplx, Nx, seed=0, scale=1.0, spin2=None):
    """scale * (A A' + I) per m, Hermitian positive definite, symmetrised at columns 0 and Nx/2 (which keeps them positive definite: the average of
    two positive definite matrices); float32-representable, and still exactly symmetric after the rounding (partner entries are equal).  Complex
    blocks are spin 2 unless said otherwise."""
    spin2 = bool(cplx) if spin2 is None else spin2
    H = scale * R.case_blocks(n, Mh, cplx, seed=seed, spd=True)
    return _r32(symmetrise(H, Nx, spin2))


def cos_mask(Ny, Nx, P):
    """cosine-apodised mask in [0, 1]: 1 inside, a half-cosine edge of a fifth of each side, 0 on the border"""
    def edge(N):
        w = max(2, N // 5)
        t = np.ones(N)
        r = 0.5 * (1 - np.cos(np.pi * np.arange(w) / w))
        t[:w] = r
        t[N - w:] = r[::-1]
        return t
    m = edge(Nx)[:, None] * edge(Ny)[None, :]
    return _r32(np.broadcast_to(m, (P, Nx, Ny)).copy())


def build_case(case, seed=0, symmetric=True):
    """the operators and inputs of a case, float64 arrays holding float32-representable numbers"""
    Ny, Nx, B, spin, form = case
    P = 1 if spin == 0 else 2
    n, Mh, cplx = P * Ny, Nx // 2 + 1, spin == 2
    rng = np.random.default_rng([seed, Ny, Nx, B, spin])
    mk = (lambda s, sc: sym_spd_blocks(n, Mh, cplx, Nx, seed=s, scale=sc)) if symmetric else (lambda s, sc: _r32(sc * R.case_blocks(n, Mh, cplx, seed=s, spd=True)))
    o = {"Ny": Ny, "Nx": Nx, "P": P, "B": B, "form": form, "Cf": mk(seed + 1, 1.0), "beam": None, "M": None, "var": None, "Cn": None, "Mhat": None, "Cnhat": None}
    if form != "bare":
        o["beam"] = mk(seed + 2, 0.5)
        o["M"] = cos_mask(Ny, Nx, P)
        o["Mhat"] = float(np.float32(o["M"].mean()))
    if form == "blk":
        o["Cn"] = mk(seed + 3, 0.25)
    else:
        x, y = np.meshgrid(np.arange(Nx) / Nx, np.arange(Ny) / Ny, indexing="ij")
        wave = np.sin(2 * np.pi * x) * np.cos(np.pi * y)
        # ("bare": nothing but the noise contrast keeps the scalar-Cnhat preconditioner from being the inverse, so it is made large)
        var = 0.25 * (np.exp(2.0 * wave) if form == "bare" else 1.0 + 0.5 * wave)
        o["var"] = _r32(np.stack([var * (1 + 0.1 * k) for k in range(P)]))
        o["Cnhat"] = float(np.float32(o["var"].mean()))
    o["f"] = to_az(_r32(rng.standard_normal((B, P, Nx, Ny))), P, np.float64)          # images of maps
    o["f"] = _r32(o["f"])
    o["fstart"] = _r32(to_az(_r32(0.1 * rng.standard_normal((B, P, Nx, Ny))), P, np.float64))
    o["d"] = _r32(rng.standard_normal((B, P, Nx, Ny)))
    o["wf"], o["wn"] = _r32(rng.standard_normal((B, P, Nx, Ny))), _r32(rng.standard_normal((B, P, Nx, Ny)))     # the white draws of sample_f
    return o


# ---- bases and products in dt ---------------------------------------------------------------------------------------------------------------
def to_az(m, P, dt):
    return R.az_fwd(m, dt) if P == 1 else R.qu_fwd(m, dt)


def to_map(f, P, Nx, dt):
    return R.az_inv(f, Nx, dt) if P == 1 else R.qu_inv(f, Nx, dt)


def _c(M, dt):
    return np.asarray(M).astype(R.cdt(dt) if np.iscomplexobj(M) else dt)


def blk(M, f, dt, adjoint=False):
    return R.apply(_c(M, dt), np.asarray(f).astype(R.cdt(dt)), adjoint).astype(R.cdt(dt))


def map_dot(a, b):
    """dot(a, b) per batch slot of two map arrays (src/proj_equirect.jl:355), in double like the device's"""
    return np.array([R.field_dot(x, y) for x, y in zip(a, b)])


def az_weights(Nx, n, spin2):
    Mh = Nx // 2 + 1
    w = np.full(Mh, 1.0 if spin2 else 2.0)
    for m in ([0, Nx // 2] if Nx % 2 == 0 else [0]):
        w[m] = 0.5 if spin2 else 1.0
    return w


def az_dot(a, b, Nx, spin2):
    """the map dot formed in the Az basis: Σ w_m Re(conj(a) b)"""
    w = az_weights(Nx, a.shape[-1], spin2)
    t = (np.conj(a.astype(np.complex128)) * b.astype(np.complex128)).real
    return np.sum(t * w[None, :, None], axis=(1, 2))


def derive(o, dt):
    """the operators the device is handed, in dt: pinv in float64 rounded to dt (as BlockDiagEquiRect.pinv does on the host), the products in dt"""
    P, Nx = o["P"], o["Nx"]
    g = {"CfI": _c(R.op_pinv(o["Cf"]), dt), "beam": None if o["beam"] is None else _c(o["beam"], dt), "M": None if o["M"] is None else o["M"].astype(dt)}
    g["CnI"] = None if o["Cn"] is None else _c(R.op_pinv(o["Cn"]), dt)
    g["cni_pix"] = None if o["var"] is None else (dt(1) / o["var"].astype(dt)).astype(dt)
    # preconditioner pinv(pinv(Cf) + B^' M^' pinv(Cn^) M^ B^) (src/dataset.jl:129-132): B^ = B, M^ = Mhat (a scalar) or 1, Cn^ = Cn (block) or Cnhat (a scalar)
    mh = dt(1) if o["M"] is None else dt(o["Mhat"])
    n = g["CfI"].shape[-1]
    if g["CnI"] is not None:
        X = (g["CnI"] * (mh * mh)).astype(g["CnI"].dtype)
        if g["beam"] is not None:
            X = R.matmul(g["beam"], R.matmul(X, g["beam"]), adjA=True)
    else:
        s = dt(mh * mh) * (dt(1) / dt(o["Cnhat"]))
        X = (R.matmul(g["beam"], g["beam"], adjA=True) * s) if g["beam"] is not None else (np.eye(n, dtype=dt)[None] * s)
    tot = (g["CfI"] + X).astype(np.result_type(g["CfI"].dtype, X.dtype))
    g["PI"] = _c(R.op_pinv(tot), dt)
    g["logdet"] = float(np.real(R.op_logdet(o["Cf"]))) + (float(np.real(R.op_logdet(o["Cn"]))) if o["Cn"] is not None else
                                                          float(np.sum(np.log(o["var"])) * (P / o["var"].shape[0])))
    return g


def _mask(g, m):
    return m if g["M"] is None else (m * g["M"][None]).astype(m.dtype)


def _beam(g, f, dt, adjoint=False):
    return f if g["beam"] is None else blk(g["beam"], f, dt, adjoint)


def mean(o, g, f, dt):
    """M B f as a map"""
    return _mask(g, to_map(_beam(g, np.asarray(f).astype(R.cdt(dt)), dt), o["P"], o["Nx"], dt))


def _cn_inv(o, g, z, dt):
    """Cn⁻¹ z for a map z"""
    if g["cni_pix"] is not None:
        return (z * g["cni_pix"][None]).astype(dt)
    return to_map(blk(g["CnI"], to_az(z, o["P"], dt), dt), o["P"], o["Nx"], dt)


def _back(o, g, z, dt):
    """B' M' z in the Az basis for a map z"""
    return _beam(g, to_az(_mask(g, z), o["P"], dt), dt, adjoint=True)


def gradientf(o, g, f, d, dt):
    """B' M' Cn⁻¹ (d − M B f) − Cf⁻¹ f; f is None: f = 0; d is None: d = 0"""
    z = (0 if d is None else np.asarray(d).astype(dt)) - (0 if f is None else mean(o, g, f, dt))
    out = _back(o, g, _cn_inv(o, g, np.asarray(z, dtype=dt), dt), dt)
    return out if f is None else (out - blk(g["CfI"], f, dt)).astype(R.cdt(dt))


def logpdf(o, g, f, d, dt):
    """−½ [ (d − MBf)' Cn⁻¹ (d − MBf) + f' Cf⁻¹ f + logdet Cn + logdet Cf ] per batch slot; the sums in double like the device's"""
    z = (np.asarray(d).astype(dt) - mean(o, g, f, dt)).astype(dt)
    q1 = map_dot(z, _cn_inv(o, g, z, dt))
    fm = to_map(np.asarray(f).astype(R.cdt(dt)), o["P"], o["Nx"], dt)
    q2 = map_dot(fm, to_map(blk(g["CfI"], f, dt), o["P"], o["Nx"], dt))
    return -0.5 * (q1 + q2 + g["logdet"])


def hessian(o, g, p, dt):
    """(Cf⁻¹ + B' M' Cn⁻¹ M B) p in the Az basis"""
    return (blk(g["CfI"], p, dt) + _back(o, g, _cn_inv(o, g, mean(o, g, p, dt), dt), dt)).astype(R.cdt(dt))


def preconditioner(o, g, r, dt):
    return blk(g["PI"], r, dt)


def rhs(o, g, d, dt):
    return _back(o, g, _cn_inv(o, g, np.asarray(d).astype(dt), dt), dt)


def wiener(o, g, d, dt, fstart=None, nsteps=NSTEPS, tol=0.0):
    """argmaxf_logpdf with MAP-held vectors and the map dot (the reference's bases): (f in the Az basis, history (nit, B))"""
    P, Nx = o["P"], o["Nx"]
    az, mp = (lambda m: to_az(m, P, dt)), (lambda f: to_map(f, P, Nx, dt))
    b = mp(rhs(o, g, d, dt))
    x0 = np.zeros_like(b) if fstart is None else mp(np.asarray(fstart).astype(R.cdt(dt)))
    x, hist = conjugate_gradient(lambda r: mp(preconditioner(o, g, az(r), dt)), lambda p: mp(hessian(o, g, az(p), dt)), b, x0, map_dot, nsteps, tol)
    return az(x), np.array([h[1] for h in hist], dtype=np.float64)


def simulate(o, g, wf, wn, dt):
    """(f, d) = (sqrt(Cf) wf, M B f + sqrt(Cn) wn) from white maps (src/dataset.jl:49-57); sqrt in float64 rounded to dt like BlockDiagEquiRect.sqrt"""
    P, Nx = o["P"], o["Nx"]
    f = blk(R.op_sqrt(o["Cf"]), to_az(np.asarray(wf).astype(dt), P, dt), dt)
    if o["Cn"] is not None:
        noise = to_map(blk(R.op_sqrt(o["Cn"]), to_az(np.asarray(wn).astype(dt), P, dt), dt), P, Nx, dt)
    else:
        noise = (np.asarray(wn).astype(dt) * np.sqrt(o["var"].astype(dt))[None]).astype(dt)
    return f, (mean(o, g, f, dt) + noise).astype(dt)


def sample_f(o, g, d, wf, wn, dt, nsteps=NSTEPS, tol=0.0):
    """sim.f + argmaxf_logpdf(d - sim.d) (src/maximization.jl:56-62)"""
    sf, sd = simulate(o, g, wf, wn, dt)
    f, hist = wiener(o, g, (np.asarray(d).astype(dt) - sd).astype(dt), dt, nsteps=nsteps, tol=tol)
    return (sf + f).astype(R.cdt(dt)), hist


def wiener_az(o, g, d, dt, fstart=None, nsteps=NSTEPS, tol=0.0):
    """the same with the vectors held in the Az basis and the weighted dot, as the device does"""
    spin2 = o["P"] == 2
    b = rhs(o, g, d, dt)
    x0 = np.zeros_like(b) if fstart is None else np.asarray(fstart).astype(R.cdt(dt))
    x, hist = conjugate_gradient(lambda r: preconditioner(o, g, r, dt), lambda p: hessian(o, g, p, dt), b, x0, lambda u, v: az_dot(u, v, o["Nx"], spin2), nsteps, tol)
    return x, np.array([h[1] for h in hist], dtype=np.float64)


# ---- what the GPU tests compare, per case ---------------------------------------------------------------------------------------------------
SCALARS = ("logpdf", "hist", "hist_fs")


def reference(case, dt):
    """every compared quantity of a case, computed in dt"""
    o = build_case(case)
    g = derive(o, dt)
    out = {"mean": mean(o, g, o["f"], dt), "grad": gradientf(o, g, o["f"], o["d"], dt), "grad_f0": gradientf(o, g, None, o["d"], dt),
           "grad_d0": gradientf(o, g, o["f"], None, dt), "logpdf": logpdf(o, g, o["f"], o["d"], dt)}
    out["f_cg"], out["hist"] = wiener(o, g, o["d"], dt)
    out["f_cg_fs"], out["hist_fs"] = wiener(o, g, o["d"], dt, fstart=o["fstart"])
    # the stop rule: tol at the float64 run's 5th residual maximum, raised by 1e-3 of itself so that neither precision sits on the strict `res < tol`
    h64 = out["hist"] if dt == np.float64 else wiener(o, derive(o, np.float64), o["d"], np.float64)[1]
    out["tol_stop"] = float(h64[4].max()) * (1 + 1e-3)
    out["f_stop"], hs = wiener(o, g, o["d"], dt, nsteps=50, tol=out["tol_stop"])
    out["n_stop"] = len(hs)
    out["sample_f"] = sample_f(o, g, o["d"], o["wf"], o["wn"], dt)[0]
    return out


def distance(q, a, b):
    """of a from the reference b: the largest relative error for per-slot scalars, relative L2 for fields"""
    a, b = np.asarray(a), np.asarray(b)
    if q in SCALARS:
        return float(np.max(np.abs(a - b) / np.abs(b)))
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


# ---- the reference's own test size with Cf = Cℓ_to_Cov (test/runtests.jl:629-630): 32 x 64, B = 2 -------------------------------------------
CL_NY, CL_NX, CL_B = 32, 64, 2


def cl_case(spin, Cf):
    """the "pix" operators of (32, 64, B = 2) around the given covariance blocks (the device's Cℓ_to_Cov downloaded, or its NumPy restatement for the
    budget): noise variance and data scaled to the signal's level, so that the filter is neither the data nor zero"""
    o = build_case((CL_NY, CL_NX, CL_B, spin, "pix"))
    o["Cf"] = np.asarray(Cf)
    s = float(np.float32(np.mean(np.abs(np.diagonal(o["Cf"], axis1=1, axis2=2)))))
    o["var"] = _r32(o["var"] * s * 4)
    o["Cnhat"] = float(np.float32(o["var"].mean()))
    o["d"] = _r32(o["d"] * np.sqrt(s))
    return o


def cl_reference(o, dt):
    f, h = wiener(o, derive(o, dt), o["d"], dt)
    return {"f_cg": f, "hist": h}


def cl_blocks_numpy(spin):
    """Cℓ_to_Cov(:I / :P) at the reference's test geometry by tests/_equirect_cov_ref.py, float32-representable"""
    import _equirect_cov_ref as V
    tt, ee, bb = V.camb_total(V.LMAX_TEST)
    th = R.geometry(CL_NY, CL_NX, V.REF_THETA_SPAN, V.REF_PHI_SPAN)["theta"]
    return _r32(V.cov_I(th, V.REF_PHI_SPAN, CL_NX, tt) if spin == 0 else V.cov_P(th, V.REF_PHI_SPAN, CL_NX, ee, bb))
