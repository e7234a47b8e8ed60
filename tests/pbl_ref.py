"""NumPy restatement of the simple-physics surface fluxes and boundary layer (libmpasdyn k_pbl.hip; the formulas are
stated in include/mpas_dyn.h, mpas_atm_surface_pbl): the authority the GPU task is tested against.  No reference
task exists -- the scheme is the surface-flux and boundary-layer part of the simple-physics package of Reed &
Jablonowski (2012), on the model's own layers and layer mass instead of pressure thicknesses, with the mixing ratio
qv where the source has specific humidity; its large-scale condensation is left to the Kessler task.  Every
expression is written in the kernel's operand order (no fused multiply-add on either side), the two switches (Cd at
20 m/s, the mixing's decay above 850 hPa) are selects on the kernel's comparisons, and the two tridiagonal systems
are solved by the Thomas algorithm in the one order `thomas` states: the device's exp, sqrt and pow against NumPy's
are the only differences.

`columns` is the scheme on plain [n, L] arrays (the CPU properties of tests/test_pbl.py run on it); `surface_pbl`
applies it to a HostState as the task does, `project_edges` is the task's edge kernel.  Also here: the generator of
physical test columns."""
import math

import numpy as np

RGAS = 287.0
CP_DRY = 3.5 * RGAS
P0 = 1.0e5
GRAVITY = 9.80616
RV = 461.6
RVORD = RV / RGAS
CD0, CD1, CDMAX, WIND_SW = 7.0e-4, 6.5e-5, 2.0e-3, 20.0
CH = 1.1e-3
P_TOP, P_STRATO = 85000.0, 10000.0  # the mixing is full below 850 hPa and decays with a 100 hPa scale above
EPS, E0, LV_RV, T00 = 0.622, 610.78, 2.5e6 / 461.5, 273.16


def thomas(a, b, c, d):
    """a(k) x(k-1) + b(k) x(k) + c(k) x(k+1) = d(k) on [n, L] arrays (a(0) and c(L-1) multiply nothing: the level
    below 0 reads 0), the one order of the kernel: forward with cp(-1) = dp(-1) = 0
        al = 1 / (b(k) - a(k) cp(k-1));   cp(k) = c(k) al;   dp(k) = (d(k) - a(k) dp(k-1)) al
    (one reciprocal per level, shared by every right-hand side of the system), then back from x(L-1) = dp(L-1):
    x(k) = dp(k) - cp(k) x(k+1)."""
    n, L = d.shape
    cp, dp = np.zeros((n, L)), np.zeros((n, L))
    cprev, dprev = np.zeros(n), np.zeros(n)
    for k in range(L):
        al = 1.0 / (b[:, k] - a[:, k] * cprev)
        cp[:, k] = c[:, k] * al
        dp[:, k] = (d[:, k] - a[:, k] * dprev) * al
        cprev, dprev = cp[:, k], dp[:, k]
    x = dp.copy()
    for k in range(L - 2, -1, -1):
        x[:, k] = dp[:, k] - cp[:, k] * x[:, k + 1]
    return x


def drag(wind):
    return np.where(wind < WIND_SW, CD0 + CD1 * wind, CDMAX)


def qsat_surface(ps, ts):
    return EPS / ps * E0 * np.exp(-LV_RV * (1.0 / ts - 1.0 / T00))


def decay(pint):
    x = (P_TOP - pint) / P_STRATO
    return np.where(pint >= P_TOP, 1.0, np.exp(-(x * x)))


def columns(dt, rdzw, zz, rz, p, pi, theta, qv, ua, va, ps, ts):
    """The scheme on n columns of L levels (level 0 the lowest): rdzw [L]; zz, rho_zz, p, pi, theta, qv, ua, va
    [n, L]; ps, ts [n].  Returns a dict of everything it forms; the results are u2, v2, th2, q2 [n, L] and E [n]."""
    dt = float(dt)
    n, L = theta.shape
    rdzw = np.asarray(rdzw)[None, :L]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = rz / rdzw
        dz = 1.0 / (rdzw * zz)
        rho_d = zz * rz
        za = 0.5 * dz[:, 0]
        wind = np.sqrt(ua[:, 0] * ua[:, 0] + va[:, 0] * va[:, 0])
        cd = drag(wind)
        qss = qsat_surface(ps, ts)
        am = cd * wind * dt / za
        ah = CH * wind * dt / za
        u1, v1, th1, q1 = ua.copy(), va.copy(), theta.copy(), qv.copy()
        u1[:, 0] = ua[:, 0] / (1.0 + am)
        v1[:, 0] = va[:, 0] / (1.0 + am)
        th1[:, 0] = (theta[:, 0] + ah * ts / pi[:, 0]) / (1.0 + ah)
        q1[:, 0] = (qv[:, 0] + ah * qss) / (1.0 + ah)
        E = m[:, 0] * (q1[:, 0] - qv[:, 0])
        # the interfaces k = 1..L-1 between levels k-1 and k; D(0) = D(L) = 0
        Dm, Dh = np.zeros((n, L + 1)), np.zeros((n, L + 1))
        pint, f = np.zeros((n, L + 1)), np.zeros((n, L + 1))
        if L > 1:
            s = dz[:, 1:] + dz[:, :-1]
            pint[:, 1:L] = (dz[:, 1:] * p[:, :-1] + dz[:, :-1] * p[:, 1:]) / s
            rhoi = (dz[:, 1:] * rho_d[:, :-1] + dz[:, :-1] * rho_d[:, 1:]) / s
            dzc = 0.5 * s
            f[:, 1:L] = decay(pint[:, 1:L])
            Dm[:, 1:L] = rhoi * cd[:, None] * wind[:, None] * za[:, None] * f[:, 1:L] / dzc
            Dh[:, 1:L] = rhoi * CH * wind[:, None] * za[:, None] * f[:, 1:L] / dzc
        out = {}
        for name, D, xs in (("m", Dm, (u1, v1)), ("h", Dh, (th1, q1))):
            a = -dt * D[:, :L] / m
            c = -dt * D[:, 1:] / m
            b = 1.0 - a - c
            out["a" + name], out["b" + name], out["c" + name] = a, b, c
            out["x" + name] = [thomas(a, b, c, x) for x in xs]
    u2, v2 = out["xm"]
    th2, q2 = out["xh"]
    return dict(out, m=m, dz=dz, rho_d=rho_d, za=za, wind=wind, cd=cd, qss=qss, am=am, ah=ah, u1=u1, v1=v1, th1=th1,
                q1=q1, E=E, Dm=Dm, Dh=Dh, pint=pint, f=f, u2=u2, v2=v2, th2=th2, q2=q2)


def surface_pressure(st):
    """the forcing task's ps, term for term (tests/forcing_ref.py: level 1 of rho_zz and qtot as found)"""
    nC = st.nCells
    dz0 = 1.0 / st["rdzw"][0]
    rq0 = st["rho_zz"][:nC, 0] * (1.0 + st["qtot"][:nC, 0])
    rq1 = st["rho_zz"][:nC, 1] * (1.0 + st["qtot"][:nC, 1])
    return 0.5 * dz0 * GRAVITY * (1.25 * rq0 - 0.25 * rq1) + st["pressure_p"][:nC, 0] + st["pressure_base"][:nC, 0]


def project_edges(st, Fu, Fv):
    """the edge kernel: tend_ru_physics = 0.5 (Fu(c1) + Fu(c2)) cosA + 0.5 (Fv(c1) + Fv(c2)) sinA on levels
    0..L-1 of every edge, ids as the library holds them (an id outside [0, n] is n; row n holds zeros); cos and
    sin are libm's, per edge, as the library takes them on the host at upload.  Fu, Fv: [nCells, L]."""
    nC, nE, L = st.nCells, st.nEdges, st.L
    ang = st["angleEdge"][:nE, 0]
    cosA = np.array([math.cos(x) for x in ang])[:, None]
    sinA = np.array([math.sin(x) for x in ang])[:, None]
    fu, fv = np.zeros((nC + 1, L)), np.zeros((nC + 1, L))
    fu[:nC], fv[:nC] = Fu, Fv
    coe = st["cellsOnEdge"][:nE]
    coe = np.where((coe < 0) | (coe > nC), nC, coe)
    return 0.5 * (fu[coe[:, 0]] + fu[coe[:, 1]]) * cosA + 0.5 * (fv[coe[:, 0]] + fv[coe[:, 1]]) * sinA


def column_inputs(st, ts):
    """`columns`' arguments behind dt, from HostState st as the task reads them"""
    nC, L = st.nCells, st.L
    qv = st["scalars"][:nC, :L, 0].copy()
    return dict(rdzw=st["rdzw"][:L].copy(), zz=st["zz"][:nC, :L].copy(), rz=st["rho_zz"][:nC, :L].copy(),
                p=st["pressure_base"][:nC, :L] + st["pressure_p"][:nC, :L], pi=st["exner"][:nC, :L].copy(),
                theta=st["theta_m"][:nC, :L] / (1.0 + RVORD * qv), qv=qv,
                ua=st["uReconstructZonal"][:nC, :L].copy(), va=st["uReconstructMeridional"][:nC, :L].copy(),
                ps=surface_pressure(st), ts=np.asarray(ts, dtype=np.float64)[:nC].copy())


def surface_pbl(st, dt, ts, acc=None):
    """The task on HostState st, in place: theta_m, rtheta_p, exner, pressure_p and scalar 0 on levels 0..L-1 of
    the cells, tend_ru_physics on levels 0..L-1 of the edges.  ts: [nCells] surface temperatures.  acc: None or
    the accumulators {"evap", "evap_last", "calls"}.  Returns `columns`' dict with Fu, Fv [nCells, L] added."""
    nC, L = st.nCells, st.L
    dt = float(dt)
    tm = st["theta_m"][:nC, :L].copy()
    rtp = st["rtheta_p"][:nC, :L].copy()
    rz = st["rho_zz"][:nC, :L]
    zz = st["zz"][:nC, :L]
    rtb = st["rtheta_base"][:nC, :L]
    exb = st["exner_base"][:nC, :L]
    qv = st["scalars"][:nC, :L, 0].copy()
    ua = st["uReconstructZonal"][:nC, :L]
    va = st["uReconstructMeridional"][:nC, :L]
    theta = tm / (1.0 + RVORD * qv)
    d = columns(dt, **column_inputs(st, ts))
    th2, q2 = d["th2"], d["q2"]
    with np.errstate(over="ignore", invalid="ignore"):
        dth = th2 - theta
        tm1 = tm + dth * (1.0 + RVORD * q2) + theta * RVORD * (q2 - qv)
        dtm = tm1 - tm
        rtp1 = rtp + rz * dtm
        ex1 = np.power(zz * (RGAS / P0) * (rtp1 + rtb), RGAS / (CP_DRY - RGAS))
        pp1 = zz * RGAS * (ex1 * rtp1 + rtb * (ex1 - exb))
        Fu = rz * (d["u2"] - ua) / dt
        Fv = rz * (d["v2"] - va) / dt
    st["theta_m"][:nC, :L] = tm1
    st["rtheta_p"][:nC, :L] = rtp1
    st["exner"][:nC, :L] = ex1
    st["pressure_p"][:nC, :L] = pp1
    st["scalars"][:nC, :L, 0] = q2
    st["tend_ru_physics"][:st.nEdges, :L] = project_edges(st, Fu, Fv)
    if acc is not None:
        acc["evap"] += d["E"]
        acc["evap_last"][...] = d["E"]
        acc["calls"] += 1.0
    return dict(d, Fu=Fu, Fv=Fv)


def new_acc(nCells):
    return {"evap": np.zeros(nCells), "evap_last": np.zeros(nCells), "calls": np.zeros(nCells)}


WRITTEN = ("theta_m", "rtheta_p", "exner", "pressure_p", "scalars", "tend_ru_physics")


def water(st):
    """per column: sum_k m qv with m = rho_zz / rdzw, kg/m2"""
    nC, L = st.nCells, st.L
    return np.sum(st["rho_zz"][:nC, :L] / st["rdzw"][:L][None, :] * st["scalars"][:nC, :L, 0], axis=1)


def physical_columns(st, seed=20120401):
    """Overwrite the task's inputs of HostState st (a helpers.make_state state, either id variant), in place, with
    physical columns; returns (st, ts).  The vertical grid thickens geometrically from 60 m to 3000 m and zz = s u
    with u uniform in 0.9..1.1 per cell and s one of 1, 0.3, 0.1, 0.03 per column, so that dz = 1 / (rdzw zz) at
    the ground runs from about 60 m to about 2 km; T = 300 K - 6.5 K/km z shifted per column by -8..+8 K and
    jittered per cell by 0.2 K, held in 200..310 K; p hydrostatic at a scale height of 8 km (850 hPa lies near
    1300 m: interfaces on both sides of it from L = 3 on), split into a base and a perturbation; rho_d = p / (R T);
    qv 0..0.02 decreasing upward, qtot = qv; the cell-centre winds a column speed of 0..40 m/s (both sides of
    20 m/s) in a random direction, sheared and jittered per level.  Every seventh column (c % 7 == 3) is calm:
    both winds +0.0 at every level.  ts is uniform in 271..302 K per column."""
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
    p = P0 * np.exp(-zmid / 8000.0)[None, :] * rng.uniform(0.98, 1.02, (nC, 1))
    pi = (p / P0) ** (RGAS / CP_DRY)
    rho_d = p / (RGAS * T)
    qv = rng.uniform(0.0, 0.02, (nC, 1)) * np.exp(-zmid / 2500.0)[None, :] * rng.uniform(0.5, 1.0, (nC, L))
    speed = rng.uniform(0.0, 40.0, (nC, 1))
    phi = rng.uniform(0.0, 2.0 * np.pi, (nC, 1))
    shear = 1.0 + rng.uniform(0.0, 1.0, (nC, 1)) * (np.arange(L)[None, :] / max(L, 1))
    ua = speed * np.cos(phi) * shear + rng.uniform(-1.0, 1.0, (nC, L))
    va = speed * np.sin(phi) * shear + rng.uniform(-1.0, 1.0, (nC, L))
    calm = CALM(nC)[:, None]
    ua, va = np.where(calm, 0.0, ua), np.where(calm, 0.0, va)
    rho_zz = rho_d / zz
    theta_m = T / pi * (1.0 + RVORD * qv)
    st["zz"][:nC, :L] = zz
    st["rho_zz"][:nC, :L] = rho_zz
    st["rho_zz"][:nC, L] = 0.9 * rho_zz[:, L - 1]  # (ps reads level 1 as found: level L at L = 1)
    st["qtot"][:nC, :L] = qv
    st["qtot"][:nC, L] = 0.0
    st["pressure_base"][:nC, :L] = 0.97 * p
    st["pressure_p"][:nC, :L] = p - st["pressure_base"][:nC, :L]
    st["exner"][:nC, :L] = pi
    st["exner_base"][:nC, :L] = pi * rng.uniform(0.99, 1.01, (nC, L))
    st["theta_m"][:nC, :L] = theta_m
    st["rtheta_base"][:nC, :L] = 0.98 * rho_zz * theta_m
    st["rtheta_p"][:nC, :L] = rho_zz * theta_m - st["rtheta_base"][:nC, :L]
    st["scalars"][:nC, :L, 0] = qv
    st["uReconstructZonal"][:nC, :L] = ua
    st["uReconstructMeridional"][:nC, :L] = va
    ts = rng.uniform(271.0, 302.0, nC)
    return st, ts


CALM = lambda nC: np.arange(nC) % 7 == 3  # noqa: E731
