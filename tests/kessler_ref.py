"""NumPy restatement of the Kessler warm-rain microphysics (libmpasdyn k_kessler.hip; the formulas are stated in
include/mpas_dyn.h, mpas_atm_kessler_microphysics): the authority the GPU task is tested against.  No reference task
exists -- the scheme is the published one of the DCMIP-2016 moist test cases (Klemp et al. 2015), with the
sedimentation as a finite-volume flux on the model's layers.  Every expression is written in the kernel's operand
order (no fused multiply-add on either side), max / min are selects on the kernel's comparisons, and the powers of
r qr are exp(a log(r qr)) on one logarithm per evaluation point, as in the kernel: the device's pow / exp / log
against NumPy's are the only differences.

Also here: the generator of physical test columns (helpers.make_state's raw random exner, zz and theta_m are no
valid atmosphere for this scheme)."""
import numpy as np

RGAS = 287.0
CP_DRY = 3.5 * RGAS
P0 = 1.0e5
RV = 461.6
RVORD = RV / RGAS
F2X = 17.27
LV = 2.5e6
CP = 1003.0
F5 = 237.3 * F2X * LV / CP
XK = 0.2875
PSL = 1000.0
MAX_SUB = 4096
ARM_RATE, ARM_DEFICIT, ARM_RAIN = 1, 2, 4  # bits of diag["arm"]: which arm of ern's min a subcycle took


def mx(a, b):
    return np.where(a > b, a, b)


def mn(a, b):
    return np.where(a < b, a, b)


def klog(y):
    """the shared logarithm of the powers of y = r qr: -inf for y <= 0, so that every power of it is 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(y > 0.0, np.log(np.where(y > 0.0, y, 1.0)), -np.inf)


def terminal_velocity(rqr, rho_d, rho_d0):
    """vt = 36.34 (r qr)^0.1364 sqrt(rho_d(0) / rho_d), the power through the shared logarithm"""
    lg = klog(np.asarray(rqr, dtype=np.float64))
    return 36.34 * np.exp(0.1364 * lg) * np.sqrt(rho_d0 / rho_d)


def saturation(T, pc):
    return pc * np.exp(F2X * (T - 273.0) / (T - 36.0))


def pc_of(pi):
    return 3.8 / (np.power(pi, 1.0 / XK) * PSL)


def kessler(st, dt, acc=None):
    """The task on HostState st, in place, on levels 0..L-1 of the cells 0..nCells-1: theta_m, rtheta_p, exner,
    pressure_p, rt_diabatic_tend and scalars 0..2.  acc: None or the accumulators {"rain", "rain_last", "calls"}
    ([nCells] arrays), updated as the task updates them.  Returns the diagnostics: per column n, x, P and
    "clip" (a max(., 0) cut a negative value in some subcycle); per cell "arm" (bits ARM_*), "cond_pos",
    "cond_neg" (a subcycle with cond > 0 / < 0), "dsum" (the summed cond - ern), "dtheta" (theta' - theta) and
    "qc_max" (the largest qc a subcycle's autoconversion saw)."""
    nC, L = st.nCells, st.L
    dt = float(dt)
    tm = st["theta_m"][:nC, :L].copy()
    rtp = st["rtheta_p"][:nC, :L].copy()
    rz = st["rho_zz"][:nC, :L]
    zz = st["zz"][:nC, :L]
    ex = st["exner"][:nC, :L].copy()
    rtb = st["rtheta_base"][:nC, :L]
    exb = st["exner_base"][:nC, :L]
    rdzw = st["rdzw"][:L][None, :]
    qv0 = st["scalars"][:nC, :L, 0].copy()
    qv, qc, qr = qv0.copy(), st["scalars"][:nC, :L, 1].copy(), st["scalars"][:nC, :L, 2].copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho_d = zz * rz
        ms = rz / rdzw
        dz = 1.0 / (rdzw * zz)
        pi = ex
        theta0 = tm / (1.0 + RVORD * qv0)
        theta = theta0.copy()
        r = 0.001 * rho_d
        lr = np.log(r)
        pc = 3.8 / (np.power(pi, 1.0 / XK) * PSL)
        srho = np.sqrt(rho_d[:, :1] / rho_d)
        lcp = LV / (CP * pi)
        lg = klog(r * qr)
        vt = 36.34 * np.exp(0.1364 * lg) * srho
        x = np.max(vt * dt / (0.8 * dz), axis=1) if L else np.zeros(nC)
        x = np.where(np.isnan(x), 0.0, x)
        n = np.where(x > 1.0, np.where(x < float(MAX_SUB), np.ceil(x), float(MAX_SUB)), 1.0).astype(np.int64)
        dt0 = (dt / n.astype(np.float64))[:, None]
        P = np.zeros(nC)
        arm = np.zeros((nC, L), dtype=np.int64)
        cond_pos = np.zeros((nC, L), dtype=bool)
        cond_neg = np.zeros((nC, L), dtype=bool)
        clip = np.zeros(nC, dtype=bool)
        dsum = np.zeros((nC, L))
        qc_max = np.full((nC, L), -np.inf)
        for j in range(int(n.max()) if nC else 0):
            act = (j < n)[:, None]
            if j:
                lg = klog(r * qr)
                vt = 36.34 * np.exp(0.1364 * lg) * srho
            F = rho_d * qr * vt
            Fup = np.concatenate([F[:, 1:], np.zeros((nC, 1))], axis=1)
            Pn = P + dt0[:, 0] * F[:, 0]
            sed = dt0 * (Fup - F) / ms
            q875 = np.exp(0.875 * (lg - lr))
            qrprod = qc - (qc - dt0 * mx(0.001 * (qc - 0.001), 0.0)) / (1.0 + dt0 * 2.2 * q875)
            qc1 = mx(qc - qrprod, 0.0)
            qr1 = mx(qr + qrprod + sed, 0.0)
            T = pi * theta
            qvs = pc * np.exp(F2X * (T - 273.0) / (T - 36.0))
            prod = (qv - qvs) / (1.0 + qvs * F5 / ((T - 36.0) * (T - 36.0)))
            lg1 = klog(r * qr1)
            e1 = dt0 * ((1.6 + 124.9 * np.exp(0.2046 * lg1)) * np.exp(0.525 * lg1) / (2.55e6 * pc / (3.8 * qvs) + 5.4e5)) * \
                mx(qvs - qv, 0.0) / (r * qvs)
            e2 = mx(-prod - qc1, 0.0)
            t12 = mn(e1, e2)
            ern = mn(t12, qr1)
            cond = mx(prod, -qc1)
            th1 = theta + lcp * (cond - ern)
            qv1 = mx(qv - cond + ern, 0.0)
            # diagnostics of the active columns
            a12 = np.where(e1 < e2, ARM_RATE, ARM_DEFICIT)
            arm |= np.where(act, np.where(t12 < qr1, a12, ARM_RAIN), 0)
            cond_pos |= act & (cond > 0.0)
            cond_neg |= act & (cond < 0.0)
            clip |= act[:, 0] & np.any((qc - qrprod < 0.0) | (qr + qrprod + sed < 0.0) | (qv - cond + ern < 0.0), axis=1)
            dsum = np.where(act, dsum + (cond - ern), dsum)
            qc_max = np.where(act, mx(qc_max, qc), qc_max)
            P = np.where(act[:, 0], Pn, P)
            theta = np.where(act, th1, theta)
            qv = np.where(act, qv1, qv)
            qc = np.where(act, qc1 + cond, qc)
            qr = np.where(act, qr1 - ern, qr)
        dth = theta - theta0
        tm1 = tm + dth * (1.0 + RVORD * qv) + theta0 * RVORD * (qv - qv0)
        dtm = tm1 - tm
        rtp1 = rtp + rz * dtm
        ex1 = np.power(zz * (RGAS / P0) * (rtp1 + rtb), RGAS / (CP_DRY - RGAS))
        pp1 = zz * RGAS * (ex1 * rtp1 + rtb * (ex1 - exb))
    st["theta_m"][:nC, :L] = tm1
    st["rtheta_p"][:nC, :L] = rtp1
    st["exner"][:nC, :L] = ex1
    st["pressure_p"][:nC, :L] = pp1
    st["rt_diabatic_tend"][:nC, :L] = dtm / dt
    st["scalars"][:nC, :L, 0] = qv
    st["scalars"][:nC, :L, 1] = qc
    st["scalars"][:nC, :L, 2] = qr
    if acc is not None:
        acc["rain"] += P
        acc["rain_last"][...] = P
        acc["calls"] += 1.0
    return dict(n=n, x=x, P=P, clip=clip, arm=arm, cond_pos=cond_pos, cond_neg=cond_neg, dsum=dsum, dtheta=dth,
                qc_max=qc_max)


def new_acc(nCells):
    return {"rain": np.zeros(nCells), "rain_last": np.zeros(nCells), "calls": np.zeros(nCells)}


WRITTEN = ("theta_m", "rtheta_p", "exner", "pressure_p", "rt_diabatic_tend", "scalars")


def near_integer(x, rel=1e-9):
    """columns whose x lies within `rel` relative of an integer >= 1: n = ceil(x) enters as an integer, so the
    device's x may fall on the other side.  x well below 1 is never near."""
    k = np.round(x)
    return (k >= 1.0) & (np.abs(x - k) <= rel * x)


def water(st):
    """per column: sum_k m (qv + qc + qr) with m = rho_zz / rdzw, kg/m2"""
    nC, L = st.nCells, st.L
    m = st["rho_zz"][:nC, :L] / st["rdzw"][:L][None, :]
    q = st["scalars"][:nC, :L, 0] + st["scalars"][:nC, :L, 1] + st["scalars"][:nC, :L, 2]
    return np.sum(m * q, axis=1)


def physical_columns(st, seed=20160601):
    """Overwrite the task's inputs of HostState st (a helpers.make_state state, either id variant), in place, with
    physical columns; returns st.  The vertical grid thickens geometrically from 60 m to 3000 m, and zz = s u with
    u uniform in 0.9..1.1 per cell and s one of 1, 0.3, 0.1, 0.03 per column, so that dz = 1 / (rdzw zz) at the
    ground runs from thin (about 60 m: n of the order of 100 at dt = 720 where it rains) to thick (n of a few);
    T = 300 K - 6.5 K/km z, shifted per column by -8..+8 K, jittered per cell by 0.2 K and held in 200..310 K; p
    hydrostatic at a scale height of 8 km, rho_d = p / (R T), about 1.2 at the ground and decreasing upward;
    qv = f qvs with f uniform in 0..1.3; qc 0 or up to 3e-3 (half the cells each).  Rain: a quarter of the columns
    none (n = 1); most of the others from the ground up to a random level, 0.2..1 times an amplitude of up to
    5e-3 (the sedimentation then keeps inside the limit n was chosen for); one column in twenty aloft only,
    above a random level with holes (rain then falls into thin layers n was not chosen for: the clipped columns).
    Every third column (c % 3 == 2) is dry: all three zero.  Every seventh (c % 7 == 3, where not dry) is
    subsaturated (qv = 0.5 qvs) without cloud or rain."""
    rng = np.random.default_rng(seed + 1000 * st.L)
    nC, L = st.nCells, st.L
    ratio = (3000.0 / 60.0) ** (1.0 / max(L - 1, 1))
    dzw = 60.0 * ratio ** np.arange(L)
    zmid = np.cumsum(dzw) - 0.5 * dzw
    rdzw = np.zeros(L + 1)
    rdzw[:L] = 1.0 / dzw
    st["rdzw"] = rdzw
    zz = np.array([1.0, 0.3, 0.1, 0.03])[rng.integers(0, 4, nC)][:, None] * rng.uniform(0.9, 1.1, (nC, L))
    T = 300.0 - 6.5e-3 * zmid[None, :] + rng.uniform(-8.0, 8.0, (nC, 1)) + rng.uniform(-0.2, 0.2, (nC, L))
    T = np.clip(T, 200.0, 310.0)
    p = P0 * np.exp(-zmid / 8000.0)[None, :] * np.ones((nC, 1))
    pi = (p / P0) ** (RGAS / CP_DRY)
    rho_d = p / (RGAS * T)
    qvs = saturation(T, pc_of(pi))
    qv = rng.uniform(0.0, 1.3, (nC, L)) * qvs
    qc = np.where(rng.random((nC, L)) < 0.5, 0.0, rng.uniform(0.0, 3e-3, (nC, L)))
    kind = rng.random(nC)  # < 0.25 no rain, < 0.95 from the ground up, else aloft
    klev = rng.integers(0, L, nC)[:, None]
    lev = np.arange(L)[None, :]
    amp = 5e-3 * rng.uniform(0.02, 1.0, (nC, 1))
    up = ((kind >= 0.25) & (kind < 0.95))[:, None] & (lev <= klev)
    aloft = (kind >= 0.95)[:, None] & (lev >= klev) & (rng.random((nC, L)) < 0.7)
    qr = np.where(up, rng.uniform(0.2, 1.0, (nC, L)) * amp, np.where(aloft, rng.uniform(0.0, 5e-3, (nC, L)), 0.0))
    c = np.arange(nC)
    dry = (c % 3 == 2)[:, None]
    sub = ((c % 7 == 3) & (c % 3 != 2))[:, None]
    qv = np.where(sub, 0.5 * qvs, qv)
    qc = np.where(sub, 0.0, qc)
    qr = np.where(sub, 0.0, qr)
    qv, qc, qr = (np.where(dry, 0.0, a) for a in (qv, qc, qr))
    rho_zz = rho_d / zz
    theta_m = T / pi * (1.0 + RVORD * qv)
    st["zz"][:nC, :L] = zz
    st["rho_zz"][:nC, :L] = rho_zz
    st["exner"][:nC, :L] = pi
    st["exner_base"][:nC, :L] = pi * rng.uniform(0.99, 1.01, (nC, L))
    st["theta_m"][:nC, :L] = theta_m
    st["rtheta_base"][:nC, :L] = 0.98 * rho_zz * theta_m
    st["rtheta_p"][:nC, :L] = rho_zz * theta_m - st["rtheta_base"][:nC, :L]
    st["scalars"][:nC, :L, 0] = qv
    st["scalars"][:nC, :L, 1] = qc
    st["scalars"][:nC, :L, 2] = qr
    return st


DRY = lambda nC: np.arange(nC) % 3 == 2  # noqa: E731
SUBSATURATED = lambda nC: (np.arange(nC) % 7 == 3) & (np.arange(nC) % 3 != 2)  # noqa: E731
