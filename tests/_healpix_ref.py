"""Float64 NumPy restatement of the HEALPix projection of the reference (src/proj_healpix.jl), vectorised: pix2angRing, the ring bilinear
interpolation of healpy.get_interp_val (T_Healpix_Base::get_interpol), θϕ_to_ij / ij_to_θϕ / get_ψpol of ProjLambert and ProjEquiRect, the flat
bilinear interpolation of Images.jl, the Projector and both directions of project with their QU rotations.  Pixel indices are 0-based; the
fractional (i, j) are 1-based like the reference's.  HEALPix fields are (B, P, npix), maps (B, P, Nx, Ny).  tests/test_healpix_ref.py pins it.

ψ comes from tangents carried by hand through θϕ_to_ij (the reference uses ForwardDiff).  The Lambert map is written in its algebraic form:
with w = R n(θ, ϕ), i = -w_x s / Δx + Ny÷2 + ½, j = -w_y s / Δx + Nx÷2 + ½, s = sqrt(2 / (1 - w_z)) -- the reference's r = 2 cos(θ'/2),
x = -r sin ϕ', y = -r cos ϕ' with (θ', ϕ') the angles of w."""
import numpy as np

PI = np.pi


# ---- pix2angRing ----------------------------------------------------------------------------------------------------------------------
def isqrt(v):
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def cap_theta(t):
    return np.arctan2(np.sqrt(t * (2.0 - t)), 1.0 - t)


def pix2ang(nside, p=None):
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    p = np.arange(npix, dtype=np.int64) if p is None else np.asarray(p, dtype=np.int64)
    n2 = 3.0 * nside * nside
    theta, phi = np.empty(p.shape), np.empty(p.shape)
    north, south = p < ncap, p >= npix - ncap
    belt = ~north & ~south
    q = p[north]
    ring = (1 + isqrt(1 + 2 * q)) >> 1
    iphi = q + 1 - 2 * ring * (ring - 1)
    theta[north] = cap_theta(ring * ring / n2)
    phi[north] = (iphi - 0.5) * PI / (2.0 * ring)
    ip = p[belt] - ncap
    ring = ip // (4 * nside) + nside
    iphi = ip % (4 * nside) + 1
    fodd = np.where((ring + nside) & 1, 1.0, 0.5)
    theta[belt] = np.arccos((2 * nside - ring) * 2.0 / (3.0 * nside))
    phi[belt] = (iphi - fodd) * PI / (2.0 * nside)
    ip = npix - p[south]
    ring = (1 + isqrt(2 * ip - 1)) >> 1
    iphi = 4 * ring + 1 - (ip - 2 * ring * (ring - 1))
    theta[south] = PI - cap_theta(ring * ring / n2)
    phi[south] = (iphi - 0.5) * PI / (2.0 * ring)
    return theta, phi


def ring_z(nside, r):
    """closed form of cos θ of ring r = 1 ... 4 Nside - 1"""
    r = np.asarray(r, dtype=np.float64)
    cap = 1.0 - r * r / (3.0 * nside * nside)
    capS = -(1.0 - (4 * nside - r) ** 2 / (3.0 * nside * nside))
    return np.where(r < nside, cap, np.where(r <= 3 * nside, (2 * nside - r) * 2.0 / (3.0 * nside), capS))


# ---- ring interpolation --------------------------------------------------------------------------------------------------------------
def ring_info(nside, r):
    """start pixel, pixel count, colatitude, shift of the rings r (int array, values clipped into 1 ... 4 Nside - 1)"""
    r = np.clip(np.asarray(r, dtype=np.int64), 1, 4 * nside - 1)
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    n2 = 3.0 * nside * nside
    s = 4 * nside - r
    north, south = r < nside, r > 3 * nside
    nr = np.where(north, 4 * r, np.where(south, 4 * s, 4 * nside))
    sp = np.where(north, 2 * r * (r - 1), np.where(south, npix - 2 * s * (s + 1), ncap + (r - nside) * 4 * nside))
    with np.errstate(invalid="ignore"):
        th = np.where(north, cap_theta(r * r / n2), np.where(south, PI - cap_theta(s * s / n2),
                                                              np.arccos(np.clip((2 * nside - r) * 2.0 / (3.0 * nside), -1, 1))))
    shift = np.where(north | south, True, ((r - nside) & 1) == 0)
    return sp, nr, th, shift


def ring_pair(nside, r, phi):
    sp, nr, th, shift = ring_info(nside, r)
    t = phi / (2 * PI / nr) - np.where(shift, 0.5, 0.0)
    fl = np.floor(t)
    i1 = np.mod(fl.astype(np.int64), nr)
    i2 = np.where(i1 + 1 < nr, i1 + 1, 0)
    return sp + i1, sp + i2, t - fl, th


def ring_above(nside, theta):
    z = np.cos(theta)
    az = np.abs(z)
    sh = np.sin(0.5 * np.where(z > 0, theta, PI - theta))
    ir = (nside * np.sqrt(6.0 * sh * sh)).astype(np.int64)
    ir1 = np.where(az <= 2.0 / 3.0, (nside * (2.0 - 1.5 * z)).astype(np.int64), np.where(z > 0, ir, 4 * nside - ir - 1))
    return np.clip(ir1, 0, 4 * nside - 1)


def interp_weights(nside, theta, phi):
    """(pix (4, n) int64, w (4, n) float64) of get_interpol at θ in [0, π], any real ϕ"""
    theta, phi = np.atleast_1d(np.asarray(theta, dtype=np.float64)), np.atleast_1d(np.asarray(phi, dtype=np.float64))
    if np.any(~((theta >= 0) & (theta <= PI))):
        raise ValueError("theta outside [0, pi]")
    npix = 12 * nside * nside
    ir1 = ring_above(nside, theta)
    ir2 = ir1 + 1
    p0, p1, wa, th1 = ring_pair(nside, ir1, phi)
    p2, p3, wb, th2 = ring_pair(nside, ir2, phi)
    north, south = ir1 == 0, ir2 == 4 * nside
    with np.errstate(invalid="ignore", divide="ignore"):
        wt = np.where(north, theta / th2, np.where(south, (theta - th1) / (PI - th1), (theta - th1) / (th2 - th1)))
    wt = np.clip(wt, 0.0, 1.0)
    w = np.stack([(1 - wa) * (1 - wt), wa * (1 - wt), (1 - wb) * wt, wb * wt])
    pix = np.stack([p0, p1, p2, p3])
    fac = (1 - wt) * 0.25
    w[:, north] = np.stack([fac, fac, (1 - wb) * wt + fac, wb * wt + fac])[:, north]
    pix[0, north], pix[1, north] = ((p2 + 2) & 3)[north], ((p3 + 2) & 3)[north]
    fac = wt * 0.25
    w[:, south] = np.stack([(1 - wa) * (1 - wt) + fac, wa * (1 - wt) + fac, fac, fac])[:, south]
    pix[2, south], pix[3, south] = (((p0 + 2) & 3) + npix - 4)[south], (((p1 + 2) & 3) + npix - 4)[south]
    return pix, w


def interp_val(m, theta, phi):
    """healpy.get_interp_val(m, θ, ϕ) for a RING map m (..., npix)"""
    m = np.asarray(m)
    nside = int(round(np.sqrt(m.shape[-1] / 12)))
    pix, w = interp_weights(nside, theta, phi)
    return sum(w[k] * m[..., pix[k]] for k in range(4))


# ---- the Cartesian projections -------------------------------------------------------------------------------------------------------
def rotzyx(deg):
    a, b, c = np.deg2rad(np.asarray(deg, dtype=np.float64))
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return Rz @ Ry @ Rx


class Lambert:
    def __init__(self, Ny, Nx, theta_pix, rotator=(0, 90, 0)):
        self.Ny, self.Nx, self.dx, self.R = Ny, Nx, np.deg2rad(theta_pix / 60.0), rotzyx(rotator)

    def ij_to_ang(self, i, j):
        x, y = self.dx * (j - self.Nx // 2 - 0.5), self.dx * (i - self.Ny // 2 - 0.5)
        r2 = x * x + y * y
        q = np.sqrt(1.0 - 0.25 * r2)
        n = np.einsum("ba,b...->a...", self.R, np.stack([-y * q, -x * q, 0.5 * r2 - 1.0]))        # R \ w
        return np.arctan2(np.hypot(n[0], n[1]), n[2]), np.arctan2(n[1], n[0])

    def ang_to_ij(self, theta, phi, jac=False):
        st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
        w = np.einsum("ab,b...->a...", self.R, np.stack([cp * st, sp * st, ct]))
        s = np.sqrt(2.0 / (1.0 - w[2]))
        i, j = -w[0] * s / self.dx + self.Ny // 2 + 0.5, -w[1] * s / self.dx + self.Nx // 2 + 0.5
        if not jac:
            return i, j
        J = []
        for dn in (np.stack([cp * ct, sp * ct, -st]), np.stack([-sp * st, cp * st, 0 * st])):      # ∂/∂θ, ∂/∂ϕ
            d = np.einsum("ab,b...->a...", self.R, dn)
            ds = 0.5 * s / (1.0 - w[2]) * d[2]
            J.append((-(d[0] * s + w[0] * ds) / self.dx, -(d[1] * s + w[1] * ds) / self.dx))
        return i, j, (J[0][0], J[1][0], J[0][1], J[1][1])                                         # J11, J12, J21, J22

    def psi(self, theta, phi):
        _, _, (J11, J12, J21, J22) = self.ang_to_ij(theta, phi, jac=True)
        return 0.5 * (np.arctan2(J11, J21) + np.arctan2(-J22, J12) - PI)


class EquiRect:
    def __init__(self, Ny, Nx, theta_span, phi_span):
        self.Ny, self.Nx = Ny, Nx
        self.th0, self.dth = min(theta_span), abs(theta_span[1] - theta_span[0])
        self.ph0, self.dph = min(phi_span), abs(phi_span[1] - phi_span[0])

    def ij_to_ang(self, i, j):
        return self.dth / self.Ny * i + self.th0 + 0 * j, self.dph / self.Nx * j + self.ph0 + 0 * i

    def ang_to_ij(self, theta, phi):
        return (theta - self.th0) / self.dth * self.Ny, np.mod(phi - self.ph0, 2 * PI) / self.dph * self.Nx

    def psi(self, theta, phi):
        return 0.0 * (theta + phi)


# ---- flat bilinear interpolation (Images.bilinear_interpolation) -----------------------------------------------------------------------
def flat_bilinear(img, i, j):
    """img (..., Nx, Ny); 1-based fractional (i, j) (i along Ny); a corner outside the array counts as zero"""
    Nx, Ny = img.shape[-2:]
    i, j = np.asarray(i, dtype=np.float64), np.asarray(j, dtype=np.float64)
    fi, fj, ci, cj = np.floor(i), np.floor(j), np.ceil(i), np.ceil(j)
    out = 0.0
    for y, wy in ((fi, 1 - i + fi), (ci, i - fi)):
        for x, wx in ((fj, 1 - j + fj), (cj, j - fj)):
            ok = (y >= 1) & (y <= Ny) & (x >= 1) & (x <= Nx)
            v = img[..., np.clip(x.astype(np.int64) - 1, 0, Nx - 1), np.clip(y.astype(np.int64) - 1, 0, Ny - 1)]
            out = out + np.where(ok, wy * wx, 0.0) * v
    return out


# ---- QU rotations (src/proj_healpix.jl:243-244 and :332-333) ---------------------------------------------------------------------------
def rot_to_cart(Q, U, psi):
    return Q * np.cos(2 * psi) - U * np.sin(2 * psi), U * np.cos(2 * psi) + Q * np.sin(2 * psi)


def rot_to_healpix(Q, U, psi):
    return Q * np.cos(2 * psi) + U * np.sin(2 * psi), U * np.cos(2 * psi) - Q * np.sin(2 * psi)


def _rotate(f, psi, rot):
    P = f.shape[1]
    if P >= 2:
        f = f.copy()
        f[:, P - 2], f[:, P - 1] = rot(f[:, P - 2].copy(), f[:, P - 1].copy(), psi)
    return f


# ---- Projector and project ---------------------------------------------------------------------------------------------------------------
class Projector:
    def __init__(self, nside, cart):
        self.nside, self.cart, self.npix = nside, cart, 12 * nside * nside
        Ny, Nx = cart.Ny, cart.Nx
        jj, ii = np.meshgrid(np.arange(1, Nx + 1, dtype=np.float64), np.arange(1, Ny + 1, dtype=np.float64), indexing="ij")   # (Nx, Ny): Ny fastest
        self.thetas, self.phis = (a.ravel() for a in cart.ij_to_ang(ii, jj))
        self.psi_cart = cart.psi(self.thetas, self.phis)
        self.hpx_theta, self.hpx_phi = pix2ang(nside)
        self.i_all, self.j_all = cart.ang_to_ij(self.hpx_theta, self.hpx_phi)
        i, j = self.i_all, self.j_all
        self.hpx_idxs_in_patch = np.nonzero((i >= 1) & (i <= Ny) & (j >= 1) & (j <= Nx))[0]
        self.touched = np.nonzero((i > 0) & (i < Ny + 1) & (j > 0) & (j < Nx + 1))[0]
        self.is_, self.js = i[self.touched], j[self.touched]
        self.psi_hpx = cart.psi(self.hpx_theta[self.touched], self.hpx_phi[self.touched])

    def cut_margin(self):
        """smallest distance, in pixels, of a HEALPix centre from the lines the two sets are cut on"""
        Ny, Nx = self.cart.Ny, self.cart.Nx
        i, j = self.i_all, self.j_all
        near = (i > -1) & (i < Ny + 2) & (j > -1) & (j < Nx + 2)
        d = [np.abs(i[near] - v) for v in (0, 1, Ny, Ny + 1)] + [np.abs(j[near] - v) for v in (0, 1, Nx, Nx + 1)]
        return min((x.min() for x in d if x.size), default=np.inf)

    def to_cart(self, h):
        """(B, P, npix) -> (B, P, Nx, Ny)"""
        v = interp_val(np.asarray(h, dtype=np.float64), self.thetas, self.phis)
        return _rotate(v, self.psi_cart, rot_to_cart).reshape(v.shape[0], v.shape[1], self.cart.Nx, self.cart.Ny)

    def to_healpix(self, m):
        """(B, P, Nx, Ny) -> (B, P, npix)"""
        m = np.asarray(m, dtype=np.float64)
        out = np.zeros(m.shape[:2] + (self.npix,))
        out[..., self.touched] = _rotate(flat_bilinear(m, self.is_, self.js), self.psi_hpx, rot_to_healpix)
        return out
