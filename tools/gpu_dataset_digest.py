"""SHA-256 of what the flat-sky data-set layer (csrc/engine_dataset.hpp, csrc/engine_cg.hpp) returns on a fixed-seed set of small cases, one line
`case : sha256` per output.  Two builds of the library that print the same lines compute the same bits on these paths; run it on both on the same
machine (`CMBL_LIB` selects a build) and compare the logs line for line.

Power-of-two cases: 32 x 32, theta = 3', beam 3', I / P / IP, f32 and f64, border mask on and off, B = 2, and B = 17 for P (the B > 16 branch of
the fused CG), each with a LenseFlow(7) and with the identity in the L slot:
  gradientf_logpdf(f, d) ; argmaxf_logpdf(tol = 0, nsteps = 8), iterate and history ; grad_logpdf (value, grad f, with a flow grad phi too) ;
  with a flow logpdf_mixed and gradient_logpdf_mixed ; with the identity NoLensingDataSet.logpdf with its gradient.
Also 24 x 40 (any size: the composed forms) for grad_logpdf and the no-lensing logpdf, and the 32 x 32 P case with CMBL_NO_FUSED_HARM=1.

    python tools/gpu_dataset_digest.py        (profiles/dataset_digest_*.txt are runs of it)"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cmblensing_jl_amd as C      # noqa: E402
from bench import synthetic_cls    # noqa: E402

THETA, BEAM, PM, NSTEPS = 3.0, 3.0, dict(pad_deg=0.2, apod_deg=0.3), 8
DT = {"f32": torch.float32, "f64": torch.float64}


def sha(a):
    a = a.arr if isinstance(a, C.Field) else a
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def say(case, what, a):
    print(f"{case} {what} : {sha(a)}", flush=True)


def say_solve(case, solve):
    """argmaxf_logpdf(tol = 0, nsteps = 8).  Without a mask the preconditioner is the inverse of the operator and the residual of step 2 is exactly 0
    in float32: the solve past it ends with CMBL_ERR_NAN, which is then the line, and the solve at the default tol (it stops there) is digested too"""
    for name, kw in (("argmaxf_logpdf", dict(tol=0.0)), ("argmaxf_logpdf(default tol)", {})):
        try:
            fw, hist = solve(nsteps=NSTEPS, **kw)
        except C.CmblError as e:
            print(f"{case} {name} : error {e.code}", flush=True)
            continue
        say(case, name + ".f", fw), say(case, name + ".hist", np.array([r for _, r in hist]))
        return


def flow_case(case, shape, pol, prec, mask, B, pow2=True):
    s = C.load_sim(THETA, shape, pol, synthetic_cls(), T=DT[prec], beam_fwhm=BEAM, pixel_mask=PM if mask else None, Nbatch=B, Nphi="flat")
    ds, p, f, d = s["ds"], s["proj"], s["f"], s["d"]
    phi1 = C.Field(p, s["phi"].arr[:1].contiguous(), C.FOURIER)
    lp, gf, gp = ds.grad_logpdf(f, phi1, d)
    say(case, "grad_logpdf.lp", lp), say(case, "grad_logpdf.gf", gf), say(case, "grad_logpdf.gphi", gp)
    if not pow2:
        return
    say(case, "gradientf_logpdf", ds.gradientf_logpdf(f, phi1, d))
    say_solve(case, lambda **kw: ds.argmaxf_logpdf(phi1, d=d, **kw))
    say(case, "logpdf_mixed", ds.logpdf_mixed(s["ftilde"], s["phi"]))
    lp, gfo, gpo = ds.gradient_logpdf_mixed(s["ftilde"], s["phi"])
    say(case, "gradient_logpdf_mixed.lp", lp), say(case, "gradient_logpdf_mixed.gf", gfo), say(case, "gradient_logpdf_mixed.gphi", gpo)


def identity_case(case, shape, pol, prec, mask, B, pow2=True):
    kw = dict(T=DT[prec], beam_fwhm=BEAM, pixel_mask=PM if mask else None, Nbatch=B)
    s = C.load_nolensing_sim(THETA, shape, pol, synthetic_cls(), **kw)
    ds, f, d = s["ds"], s["f"], s["d"]
    lp, g = ds.logpdf_and_gradient(f, d)
    say(case, "nolensing.logpdf", lp), say(case, "nolensing.gradient", g)
    if not pow2:
        return
    say(case, "gradientf_logpdf", ds.gradientf_logpdf(f, d))
    say_solve(case, lambda **kw: ds.argmaxf_logpdf(d=d, **kw))
    # the identity in the L slot of a lensing data set: the value and the gradient with respect to f (it has no pullback)
    t = C.load_sim(THETA, shape, pol, synthetic_cls(), Nphi="flat", L=C.IdentityLens, **kw)
    phi0 = C.Field(t["proj"], torch.zeros_like(t["phi"].arr[:1]), C.FOURIER)
    lp, gf, _ = t["ds"].grad_logpdf(t["f"], phi0, t["d"], want_phi=False)
    say(case, "grad_logpdf.lp", lp), say(case, "grad_logpdf.gf", gf)


def main():
    print(f"# {torch.cuda.get_device_name(0)}; library {os.path.basename(os.path.dirname(C.library_path()))}/{os.path.basename(C.library_path())}", flush=True)
    pow2 = [(pol, prec, mask, 2) for pol in ("I", "P", "IP") for prec in ("f32", "f64") for mask in (True, False)]
    pow2 += [("P", prec, mask, 17) for prec in ("f32", "f64") for mask in (True, False)]
    for pol, prec, mask, B in pow2:
        tag = f"32x32 {pol} {prec} {'mask' if mask else 'nomask'} B={B}"
        flow_case(tag + " flow", (32, 32), pol, prec, mask, B)
        identity_case(tag + " identity", (32, 32), pol, prec, mask, B)
    for pol in ("I", "P", "IP"):
        for prec in ("f32", "f64"):
            tag = f"24x40 {pol} {prec} mask B=2"
            flow_case(tag + " flow", (24, 40), pol, prec, True, 2, pow2=False)
            identity_case(tag + " identity", (24, 40), pol, prec, True, 2, pow2=False)
    os.environ["CMBL_NO_FUSED_HARM"] = "1"                   # read when a context is created
    for prec in ("f32", "f64"):
        for mask in (True, False):
            tag = f"32x32 P {prec} {'mask' if mask else 'nomask'} B=2 fused_harm=0"
            flow_case(tag + " flow", (32, 32), "P", prec, mask, 2)
            identity_case(tag + " identity", (32, 32), "P", prec, mask, 2)
    del os.environ["CMBL_NO_FUSED_HARM"]


if __name__ == "__main__":
    main()
