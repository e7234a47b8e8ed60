"""NumPy restatement of the RK3 scalar transport's two tasks (include/mpas_dyn.h:
mpas_atm_advance_scalars, mpas_atm_advance_scalars_mono_rk), in the operand order of the
kernels and of oracle/mpas_oracle.c ora_mpas_advance_scalars_mono, whose statements the
monotonic task repeats.  Pinned on the CPU by tests/test_transport_rk3.py (against the oracle
and by the properties of the scheme); the reference of tests/test_gpu_transport_rk3.py.

Ids are used as the oracle uses them: row indices into arrays of n + 1 rows (row n is the
zero slot); the scratch of an id n (edge flux, R+ / R-) is 0.
"""
import numpy as np

NSC = 8
COEF3 = 0.25  # config_coef_3rd_order


def _dims(st):
    return st.nCells, st.nEdges, st.L


def _flux3(q_im2, q_im1, q_i, q_ip1, ua):
    f4 = ua * (7. * (q_i + q_im1) - (q_ip1 + q_im2)) / 12.0
    return f4 + COEF3 * np.abs(ua) * ((q_ip1 - q_im2) - 3. * (q_i - q_im1)) / 12.0


def edge_high_order(st, src):
    """u sum_j (adv_coefs_j + sign(u) adv_coefs_3rd_j) src(advCell_j, k): [nEdges + 1, L, 8],
    row nEdges zero"""
    nC, nE, L = _dims(st)
    u = st["ruAvg"][:nE, :L]
    na = st["nAdvCellsForEdge"][:nE, 0]
    adv = st["advCellsForEdge"][:nE]
    ac, ac3 = st["adv_coefs"][:nE], st["adv_coefs_3rd"][:nE]
    sgn = np.copysign(1.0, u)
    acc = np.zeros((nE, L, NSC))
    for j in range(adv.shape[1]):
        on = j < na
        if not on.any():
            continue
        wgt = ac[:, j, None] + sgn * ac3[:, j, None]
        cj = np.where(on, adv[:, j], nC)
        acc = np.where(on[:, None, None], acc + wgt[:, :, None] * src[cj][:, :L], acc)
    out = np.zeros((nE + 1, L, NSC))
    out[:nE] = u[:, :, None] * acc
    return out


def vert_high_order(st, s):
    """interface high-order flux of the columns s [nCells, L, 8]: [nCells, L + 1, 8], zero at
    interfaces 0 and L"""
    nC, nE, L = _dims(st)
    w = st["wwAvg"][:nC, :, None]
    fzm, fzp = st["fzm"], st["fzp"]
    V = np.zeros((nC, L + 1, NSC))
    for kk in range(1, L):
        if 2 <= kk <= L - 2:
            V[:, kk] = _flux3(s[:, kk - 2], s[:, kk - 1], s[:, kk], s[:, kk + 1], w[:, kk])
        else:
            V[:, kk] = w[:, kk] * (fzm[kk] * s[:, kk] + fzp[kk] * s[:, kk - 1])
    return V


def _cell_edges(st):
    """per edge slot j of every cell: (on, e, sg) -- the slot is one of the cell's edges, the edge
    id, and +1 where the cell is cellsOnEdge(e, 0), else -1"""
    nC, nE, L = _dims(st)
    eoc, coe, ne = st["edgesOnCell"][:nC], st["cellsOnEdge"], st["nEdgesOnCell"][:nC, 0]
    cells = np.arange(nC)
    for j in range(eoc.shape[1]):
        on = j < ne
        if not on.any():
            continue
        e = np.where(on, eoc[:, j], nE)
        sg = np.where(coe[e, 0] == cells, 1.0, -1.0)
        yield on, e, sg


def advance_scalars(st, dt):
    """one unlimited stage on a copy of st: scalars := the update of scalars_old over dt with the
    high-order fluxes of scalars; returns (state, rho_int [nCells, L])"""
    nC, nE, L = _dims(st)
    out = st.copy()
    s_old = st["scalars_old"][:nC, :L]
    s_flux = st["scalars"]
    ro = st["rho_zz_old_split"][:nC, :L]
    u, w = st["ruAvg"][:, :L], st["wwAvg"][:nC]
    dv = st["dvEdge"][:, 0]
    invA = st["invAreaCell"][:nC, 0][:, None]
    rdzw = st["rdzw"][None, :L]
    H = edge_high_order(st, s_flux)
    V = vert_high_order(st, s_flux[:nC, :L])
    hd = np.zeros((nC, L))
    hs = np.zeros((nC, L, NSC))
    for on, e, sg in _cell_edges(st):
        hd = np.where(on[:, None], hd + sg[:, None] * (dv[e][:, None] * u[e]), hd)
        hs = np.where(on[:, None, None], hs + sg[:, None, None] * H[e], hs)
    wi = np.zeros((nC, L + 1))  # interfaces 0 and L carry no flux
    wi[:, 1:L] = w[:, 1:L]
    D = invA * hd + rdzw * (wi[:, 1:] - wi[:, :L])
    r_i = ro - dt * D
    new = (s_old * ro[:, :, None]
           - dt * (invA[:, :, None] * hs + rdzw[:, :, None] * (V[:, 1:] - V[:, :L]))) / r_i[:, :, None]
    out["scalars"][:nC, :L] = new
    return out, r_i


def advance_scalars_mono_rk(st, dt, flux_from_old=False):
    """the monotonic task with its two high-order fluxes taken on scalars (flux_from_old: on
    scalars_old -- mpas_atm_advance_scalars_mono itself); returns the new state"""
    nC, nE, L = _dims(st)
    out = st.copy()
    so = st["scalars_old"]
    sf = so if flux_from_old else st["scalars"]
    s = so[:nC, :L]
    ro, rn = st["rho_zz_old_split"][:nC, :L, None], st["rho_zz"][:nC, :L, None]
    u = st["ruAvg"][:, :L, None]
    w = st["wwAvg"][:nC, :, None]
    dv = st["dvEdge"][:, 0]
    coe = st["cellsOnEdge"]
    invA = st["invAreaCell"][:nC, 0][:, None, None]
    rdzw = st["rdzw"][None, :L, None]
    up, um = np.fmax(u, 0.0), np.fmin(u, 0.0)
    # edges: the upwind flux of every row (the cells recompute it) and the antidiffusive flux
    lo_e = dv[:, None, None] * (up * so[coe[:, 0]][:, :L] + um * so[coe[:, 1]][:, :L])
    Ah = edge_high_order(st, sf)
    Ah[:nE] = Ah[:nE] - lo_e[:nE]
    # interfaces: upwind and antidiffusive
    hi = vert_high_order(st, sf[:nC, :L])
    lov = np.zeros((nC, L + 1, NSC))
    lov[:, 1:L] = np.fmax(w[:, 1:L], 0.0) * s[:, :L - 1] + np.fmin(w[:, 1:L], 0.0) * s[:, 1:]
    Av = hi - lov
    # upwind update, bounds, R+ / R-
    hlo = np.zeros((nC, L, NSC))
    pin, pout = np.zeros_like(hlo), np.zeros_like(hlo)
    smax, smin = s.copy(), s.copy()
    cells = np.arange(nC)
    for on, e, sg in _cell_edges(st):
        m = on[:, None, None]
        g = sg[:, None, None]
        hlo = np.where(m, hlo + g * lo_e[e], hlo)
        a = -g * Ah[e]
        pin = np.where(m, pin + np.fmax(a, 0.0), pin)
        pout = np.where(m, pout - np.fmin(a, 0.0), pout)
        oth = np.where(coe[e, 0] == cells, coe[e, 1], coe[e, 0])
        xo = so[oth][:, :L]
        smax = np.where(m, np.fmax(smax, xo), smax)
        smin = np.where(m, np.fmin(smin, xo), smin)
    smax[:, 1:] = np.fmax(smax[:, 1:], s[:, :-1])
    smin[:, 1:] = np.fmin(smin[:, 1:], s[:, :-1])
    smax[:, :-1] = np.fmax(smax[:, :-1], s[:, 1:])
    smin[:, :-1] = np.fmin(smin[:, :-1], s[:, 1:])
    lob, lot, Ab, At = lov[:, :L], lov[:, 1:], Av[:, :L], Av[:, 1:]
    su = (s * ro - dt * (hlo * invA + (lot - lob) * rdzw)) / rn
    smax = np.fmax(smax, su)
    smin = np.fmin(smin, su)
    pin_t = dt * (pin * invA + (np.fmax(Ab, 0.0) - np.fmin(At, 0.0)) * rdzw)
    pout_t = dt * (pout * invA + (np.fmax(At, 0.0) - np.fmin(Ab, 0.0)) * rdzw)
    qin, qout = (smax - su) * rn, (su - smin) * rn
    Rp = np.zeros((nC + 1, L, NSC))
    Rm = np.zeros((nC + 1, L, NSC))
    with np.errstate(divide="ignore", invalid="ignore"):
        Rp[:nC] = np.where(pin_t > 0.0, np.fmin(1.0, qin / pin_t), 0.0)
        Rm[:nC] = np.where(pout_t > 0.0, np.fmin(1.0, qout / pout_t), 0.0)
    # the limited antidiffusive fluxes
    hc = np.zeros((nC, L, NSC))
    for on, e, sg in _cell_edges(st):
        A = Ah[e]
        c1, c2 = np.minimum(coe[e, 0], nC), np.minimum(coe[e, 1], nC)
        C = np.where(A >= 0.0, np.fmin(Rm[c1], Rp[c2]), np.fmin(Rp[c1], Rm[c2]))
        hc = np.where(on[:, None, None], hc + sg[:, None, None] * (C * A), hc)
    fc = np.zeros((nC, L + 1, NSC))  # interface kk between levels kk - 1 (below) and kk
    A = Av[:, 1:L]
    fc[:, 1:L] = np.where(A >= 0.0, np.fmin(Rm[:nC, :L - 1], Rp[:nC, 1:]), np.fmin(Rp[:nC, :L - 1], Rm[:nC, 1:])) * A
    out["scalars"][:nC, :L] = su - dt * (hc * invA + (fc[:, 1:] - fc[:, :L]) * rdzw) / rn
    return out


def rk3_transport(st, dt):
    """transport = 2 of mpas_atm_srk3 from scalars_old = scalars: two unlimited stages over dt/3
    and dt/2, then the monotonic task over dt"""
    a = st.copy()
    a["scalars_old"][...] = a["scalars"]
    a, _ = advance_scalars(a, dt / 3)
    a, _ = advance_scalars(a, dt / 2)
    return advance_scalars_mono_rk(a, dt)


def stream_flow_state(mesh, make_state, L=3, U=25.0):
    """The convergence set-up: a discretely non-divergent solid-body flow from the stream function
    psi = U R sin(lat) on the vertices, ruAvg(e,k) = U R (sin latV(v2) - sin latV(v1)) / dvEdge
    (1 + 0.3 k), wwAvg = 0, rho = 1, and the smooth field 0.01 + 0.005 cos lat cos lon in both
    time levels of all 8 scalars."""
    from mpasdyn import mesh as M
    m0 = M.zero_based(mesh)
    st = make_state(m0, L, "physical")
    nC, nE = st.nCells, st.nEdges
    dv = st["dvEdge"][:nE, 0]
    R = float(np.median(dv / np.asarray(mesh.dvEdge, dtype=np.float64)))  # the state's sphere radius
    voe = st["verticesOnEdge"][:nE]
    latv = np.asarray(mesh.latVertex, dtype=np.float64)
    psi = U * R * (np.sin(latv[voe[:, 1]]) - np.sin(latv[voe[:, 0]])) / dv
    st["ruAvg"][...] = 0.0
    st["ruAvg"][:nE, :L] = psi[:, None] * (1 + 0.3 * np.arange(L))[None, :]
    st["wwAvg"][...] = 0.0
    st["rho_zz_old_split"][:nC, :L] = 1.0
    st["rho_zz"][:nC, :L] = 1.0
    lat, lon = st["lat"][:nC, 0], st["lon"][:nC, 0]
    f = 0.01 + 0.005 * np.cos(lat) * np.cos(lon)
    for name in ("scalars", "scalars_old"):
        st[name][...] = 0.0
        st[name][:nC, :L] = f[:, None, None]
    return st


def convergence_ratios(run_steps, Ns=(8, 16, 32), T=16 * 3600.0):
    """run_steps(N, dt) -> scalars [nCells, L, 8] after N steps of dt; the two ratios of
    max|s_N - s_2N| over Ns (8: third order in time, 4: second), and the differences"""
    sol = {}
    for N in sorted({n for N in Ns for n in (N, 2 * N)}):
        sol[N] = run_steps(N, T / N)
    d = [float(np.max(np.abs(sol[N] - sol[2 * N]))) for N in Ns]
    return [d[i] / d[i + 1] for i in range(len(d) - 1)], d
