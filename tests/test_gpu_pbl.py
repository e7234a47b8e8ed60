"""GPU (libmpasdyn k_pbl.hip) surface fluxes and boundary layer: the task mpas_atm_surface_pbl against its NumPy
restatement (tests/pbl_ref.py, pinned on the CPU by tests/test_pbl.py), its surface temperature and evaporation
accumulators, and option pbl = 1 of mpas_atm_srk3.

Task parity: every written field -- theta_m, rtheta_p, exner, pressure_p, qv on its own, and tend_ru_physics through
the edge kernel -- and the two evaporation accumulators within the project's per-task bound RTOL_FAST = 1e-11 of that
field's largest magnitude; the device's exp / sqrt / pow against the host's are the only differences.  No column is
left out: both switches of the scheme are continuous.  The call counter is bit for bit; calm columns keep theta_m,
rtheta_p and qv bit for bit and get E = +0.0, and an edge between two calm cells gets tend_ru_physics = 0; every
field the task does not write is bit-unchanged, as are scalars 1..7, level L and the zero slot of what it writes.
The observed maxima are printed and recorded in DESIGN.md §7.  Everything else here is bit for bit."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle as O
import pbl_ref as P
from helpers import compare_states, make_state
from mpasdyn import decomp, jw, lib, stats, surface
from mpasdyn import mesh as M
from mpasdyn import tasks as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

RTOL_FAST = 1e-11
DT = 720.0
BOUNDS_LIB = os.path.join(REPO, "mpas-regent_amd", "mpasdyn", "libmpasdyn_bounds.so")
# one level (the surface step alone); the first interface; the smallest column with an interior level; LP 8 with
# eight columns per wavefront; LP 32 with two; the benchmark's L (the level-pair layout); level L in the last lane
LEVELS = [1, 2, 3, 5, 26, 56, 63]
EINVAL = "(-1)"
ACC = ("evap", "evap_last", "calls")
PACC = ("rain", "rain_last", "calls")

_ST = {}


def state(mesh, L, variant):
    """(state, surface temperatures), built once and never modified: "random" (raw 1-based ids) and "mpas0"
    (0-based ids) carry the generator's physical columns; "moist" is the driver's moist Jablonowski-Williamson state
    with MPAS-A's initial diagnostics (cell-centre winds included), qc = 2e-3 and qr = 1e-3 below 3 km so that it
    rains, tend_ru_physics = 0, over the sea-surface temperature of Thatcher & Jablonowski (2016)"""
    key = (L, variant)
    if key not in _ST:
        if variant == "moist":
            m0 = M.zero_based(mesh)
            st = jw.jw_state(m0, L, perturb=True)
            o = O.Oracle(st)
            o.mpas_solve_diagnostics(0, -1)
            o.mpas_reconstruct_2d(False, True)
            jw.add_moisture(st, m0)
            nC = st.nCells
            z = 0.5 * (st["zgrid"][:nC, 1:L + 1] + st["zgrid"][:nC, :L])
            low = (z < 3000.0) | (np.arange(L)[None, :] == 0)
            st["scalars"][:nC, :L, 1] = np.where(low, 2e-3, 0.0)
            st["scalars"][:nC, :L, 2] = np.where(low, 1e-3, 0.0)
            st["rt_diabatic_tend"][...] = 0.0
            st["tend_ru_physics"][...] = 0.0
            _ST[key] = (st, surface.sst_tj16(np.asarray(m0.latCell)))
        else:
            _ST[key] = P.physical_columns(make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random"))
    return _ST[key]


def gpu(st, ts, fn, opts=None, sigma=None):
    """fn(ctx) on a fresh physics-2 context holding st over the surface temperatures ts; returns what fn returns
    and the downloaded state"""
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        if os.environ.get("MPAS_LIB") == BOUNDS_LIB:  # (the child run of the bounds test)
            assert ctx.get_option("bounds") == 1, "not the bounds-checked build"
        ctx.set_option("physics", 2)
        if ts is not None:
            T.surface_set_temperature(ctx, ts)
        if sigma is not None:
            T.sigma_stats_configure(ctx, sigma)
        for k, v in (opts or {}).items():
            ctx.set_option(k, v)
        ctx.upload(st)
        out = fn(ctx)
        ctx.sync()
        ctx.download(got)
    return out, got


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_acc(a, b, names=ACC):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in names) and set(a) == set(b) == set(names)


def one_call(ctx, dt=DT):
    T.atm_surface_pbl(ctx, dt)
    return T.surface_flux_read(ctx)


def _steps(c, n=1):
    for _ in range(n):
        T.atm_srk3(c, DT, 1)


def check_task(st, ts, dt, label):
    nC, nE, L = st.nCells, st.nEdges, st.L
    ref, racc = st.copy(), P.new_acc(nC)
    d = P.surface_pbl(ref, dt, ts, racc)
    acc, got = gpu(st, ts, lambda c: one_call(c, dt))
    worst = {}

    def close(name, g, r):
        assert np.isfinite(r).all() and np.isfinite(g).all(), name
        scale = float(np.max(np.abs(r)))
        err = float(np.max(np.abs(g - r)))
        worst[name] = err / scale if scale else err
        return name, err, scale
    checks = [close(name, got[name][:nC, :L], ref[name][:nC, :L]) for name in ("theta_m", "rtheta_p", "exner", "pressure_p")]
    checks.append(close("qv", got["scalars"][:nC, :L, 0], ref["scalars"][:nC, :L, 0]))
    checks.append(close("tend_ru_physics", got["tend_ru_physics"][:nE, :L], ref["tend_ru_physics"][:nE, :L]))
    checks.append(close("evap", acc["evap"], racc["evap"]))
    checks.append(close("evap_last", acc["evap_last"], racc["evap_last"]))
    print(f"{label}: every column compared; max|gpu - restatement| / max|field|: " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, err, scale in checks:
        assert scale > 0.0 and err <= RTOL_FAST * scale, f"{name} off by {err:.3e} = {err / scale:.3e} of its max"
    assert np.array_equal(acc["calls"], racc["calls"]) and np.all(acc["calls"] == 1.0)
    assert np.array_equal(bits(acc["evap"]), bits(acc["evap_last"]))  # (the first call: 0.0 + E)
    # the task did something
    assert np.any(ref["theta_m"][:nC, :L] != st["theta_m"][:nC, :L]) and np.any(racc["evap"] != 0.0)
    # calm columns: bit for bit, as on the CPU; an edge between two calm cells (or a calm cell and the zero slot) gets 0
    calm = P.CALM(nC)
    for name in ("theta_m", "rtheta_p"):
        assert np.array_equal(bits(got[name][:nC, :L][calm]), bits(st[name][:nC, :L][calm])), name
    assert np.array_equal(bits(got["scalars"][:nC, :L, 0][calm]), bits(st["scalars"][:nC, :L, 0][calm]))
    assert np.all(bits(acc["evap"][calm]) == 0)
    calmz = np.append(calm, True)
    coe = st["cellsOnEdge"][:nE]
    coe = np.where((coe < 0) | (coe > nC), nC, coe)
    still = calmz[coe[:, 0]] & calmz[coe[:, 1]]
    if L > 1 or still.any():
        assert np.all(got["tend_ru_physics"][:nE, :L][still] == 0.0)
    # nothing else is written: every other field, scalars 1..7, and level L and the zero slot of the outputs
    bad = compare_states(got, st, rtol=0.0, skip=set(P.WRITTEN))
    assert not bad, bad[:6]
    assert np.array_equal(bits(got["scalars"][..., 1:]), bits(st["scalars"][..., 1:]))
    for name in P.WRITTEN:
        n = nE if name == "tend_ru_physics" else nC
        assert np.array_equal(bits(got[name][:, L]), bits(st[name][:, L])), name
        assert np.array_equal(bits(got[name][n]), bits(st[name][n])), name


@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("L", LEVELS)
def test_task(x1_2562, L, variant):
    st, ts = state(x1_2562, L, variant)
    check_task(st, ts, DT, f"L={L} {variant}")


@pytest.mark.parametrize("dt", [90.0, 1800.0])
def test_task_other_steps(x1_2562, dt):
    st, ts = state(x1_2562, 26, "mpas0")
    check_task(st, ts, dt, f"L=26 mpas0 dt={dt:g}")


def test_two_calls_add(x1_2562):
    st, ts = state(x1_2562, 26, "mpas0")

    def fn(c):
        a = one_call(c)
        b = one_call(c)
        T.surface_flux_reset(c)
        return a, b, T.surface_flux_read(c)
    (a, b, z), _ = gpu(st, ts, fn)
    assert np.any(a["evap_last"] != 0.0) and np.any(b["evap_last"] != a["evap_last"])
    assert np.array_equal(bits(b["evap"]), bits(a["evap_last"] + b["evap_last"]))
    assert np.all(a["calls"] == 1.0) and np.all(b["calls"] == 2.0)
    assert all(np.all(bits(z[k]) == 0) for k in ACC)


def test_a_new_surface_temperature_is_read(x1_2562):
    st, ts = state(x1_2562, 5, "mpas0")

    def fn(c):
        T.surface_set_temperature(c, ts + 3.0)
        return one_call(c)
    a, _ = gpu(st, ts, one_call)
    b, got = gpu(st, ts, fn)
    ref = st.copy()
    P.surface_pbl(ref, DT, ts + 3.0)
    live = ~P.CALM(st.nCells)
    assert np.all(b["evap"][live] > a["evap"][live])
    assert float(np.max(np.abs(got["theta_m"] - ref["theta_m"]))) <= RTOL_FAST * float(np.max(np.abs(ref["theta_m"])))


@pytest.mark.parametrize("combo", [(2, 1), (0, 0), (2, 0), (0, 1)], ids=lambda c: f"transport{c[0]}-microphysics{c[1]}")
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("L", [5, 56])
def test_step_is_the_composition(x1_2562, L, exact, combo):
    """atm_srk3 with pbl = 1 == atm_srk3 with pbl = 0, then the task: bit for bit in every field and accumulator"""
    st, ts = state(x1_2562, L, "moist")
    opts = {"exact": exact, "transport": combo[0], "microphysics": combo[1]}

    def step(c):
        _steps(c)
        return T.surface_flux_read(c), T.precip_read(c)

    def composed(c):
        _steps(c)
        return one_call(c), T.precip_read(c)
    (acc, pacc), got = gpu(st, ts, step, dict(opts, pbl=1))
    (racc, rpacc), ref = gpu(st, ts, composed, dict(opts, pbl=0))
    assert np.any(acc["evap"] != 0.0) and np.all(acc["calls"] == 1.0)
    assert np.any(got["tend_ru_physics"] != 0.0)
    assert same_acc(acc, racc) and same_acc(pacc, rpacc, PACC)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def test_step_sample_sees_the_adjusted_state(x1_2562):
    """with stats_every = 1 the step's sample comes after the task"""
    st, ts = state(x1_2562, 26, "moist")
    sigma = list(stats.DEFAULT_SIGMA)

    def step(c):
        _steps(c)
        return T.sigma_stats_read(c)

    def composed(c):
        _steps(c)
        T.atm_surface_pbl(c, DT)
        T.atm_sigma_stats_accumulate(c)
        return T.sigma_stats_read(c)
    a, got = gpu(st, ts, step, {"transport": 2, "pbl": 1, "stats_every": 1}, sigma=sigma)
    b, ref = gpu(st, ts, composed, {"transport": 2}, sigma=sigma)
    c, _ = gpu(st, ts, step, {"transport": 2, "stats_every": 1}, sigma=sigma)
    assert a["n"].max() == 1.0 and set(a) == set(b)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
    assert not np.array_equal(a["T"], c["T"])  # (the sample of the unadjusted state differs)
    assert not compare_states(got, ref, rtol=0.0)


def test_second_step_consumes_the_tendency(x1_2562):
    """tend_ru_physics after step 1 is the by-hand task's, the next step's three stages read it: two steps with the
    option == step, task, step, task; and the tendency changes what the second step computes"""
    st, ts = state(x1_2562, 26, "moist")
    keep = {}

    def two(c):
        _steps(c)
        c.sync()
        one = st.copy()
        c.download(one, names=["tend_ru_physics"])
        keep["step"] = one["tend_ru_physics"].copy()
        _steps(c)
        return T.surface_flux_read(c)

    def by_hand(c):
        _steps(c)
        T.atm_surface_pbl(c, DT)
        c.sync()
        one = st.copy()
        c.download(one, names=["tend_ru_physics"])
        keep["hand"] = one["tend_ru_physics"].copy()
        _steps(c)
        return one_call(c)

    def no_tendency(c):  # the second step without the first step's tendency
        _steps(c)
        T.atm_surface_pbl(c, DT)
        zero = st.copy()
        zero["tend_ru_physics"][...] = 0.0
        c.upload(zero, names=["tend_ru_physics"])
        _steps(c)
    acc, got = gpu(st, ts, two, {"transport": 2, "pbl": 1})
    racc, ref = gpu(st, ts, by_hand, {"transport": 2})
    _, other = gpu(st, ts, no_tendency, {"transport": 2})
    assert np.any(keep["step"] != 0.0) and np.array_equal(bits(keep["step"]), bits(keep["hand"]))
    assert np.all(acc["calls"] == 2.0) and same_acc(acc, racc)
    assert not compare_states(got, ref, rtol=0.0)
    assert not np.array_equal(other["u"], ref["u"])


def test_graph_replay_and_recapture(x1_2562):
    st, ts = state(x1_2562, 26, "moist")
    out, accs = {}, {}
    for graph in (0, 1):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("graph", graph)
            ctx.set_option("physics", 2)
            T.surface_set_temperature(ctx, ts)
            ctx.set_option("transport", 2)
            ctx.set_option("microphysics", 1)
            ctx.set_option("pbl", 1)
            ctx.upload(st)
            _steps(ctx, 2)
            ctx.sync()
            assert ctx.get_option("graph_captures") == graph
            assert ctx.get_option("graph_launches") == 2 * graph
            ctx.download(got)
            accs[graph] = T.surface_flux_read(ctx)
            if graph:
                ctx.set_option("pbl", 0)  # toggling the option: a new capture
                _steps(ctx, 1)
                ctx.sync()
                assert ctx.get_option("graph_captures") == 2
                assert np.all(T.surface_flux_read(ctx)["calls"] == 2.0)  # (no task in that step)
                ctx.set_option("pbl", 1)
                ctx.timing(True)  # the task appears in the per-task timing, once per step, behind Kessler's
                _steps(ctx, 1)
                ctx.sync()
                rep = ctx.timing_report()
                assert rep["atm_surface_pbl"][0] == 1 and rep["atm_kessler_microphysics"][0] == 1, rep
                rows = [k for k, (calls, _ms) in rep.items() if calls > 0]
                assert rows.index("atm_surface_pbl") > rows.index("atm_kessler_microphysics")
        out[graph] = got
    assert np.all(accs[1]["calls"] == 2.0) and np.any(accs[1]["evap"] != 0.0)
    assert same_acc(accs[1], accs[0])
    bad = compare_states(out[1], out[0], rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("name", ["L5;physics=2", "L56;physics=2", "L5;physics=2,transport=2", "L56;physics=2,forcing=1"])
def test_rows_without_the_option_are_the_recorded_ones(name):
    """a step with pbl = 0 makes the launches recorded before the feature (tools/record_step_rows.py's record)"""
    import json

    import record_step_rows as R
    with open(R.FIXTURE) as f:
        fx = json.load(f)
    L, opts, dt, schedule, dec = R.CONFIGS[name]
    want = R.unpack_steps(fx, name)
    assert R.step_rows((L, tuple(opts) + (("pbl", 0),), dt, schedule, dec)) == want
    assert not any(k == "atm_surface_pbl" for s in want for k, _ in s)


def _run_parts(st, ts, nparts, overlap, fn):
    """fn on nparts loopback subdomains, one host thread each (the setup of tests/test_gpu_decomp.py's
    run_decomposed); returns the accumulators in global cell order and the assembled state"""
    d = decomp.Decomposition(st, nparts)
    locs = [d.local_state(r) for r in range(nparts)]
    ctxs = [lib.Context(*d.n_local(r), st.L) for r in range(nparts)]
    parts, errs = [None] * nparts, [None] * nparts
    try:
        for r, c in enumerate(ctxs):
            c.set_option("overlap", overlap)
            lib.setup_subdomain(c, d, r)
            c.upload(locs[r])
            c.set_option("physics", 2)
            T.surface_set_temperature(c, ts[d.global_ids(r)["cell"]])
        lib.halo_loopback(ctxs)

        def drive(r):
            try:
                fn(ctxs[r])
                ctxs[r].sync()
                parts[r] = T.surface_flux_read(ctxs[r], d.n_owned(r)[0])
            except Exception as e:  # noqa: BLE001 -- reported below
                errs[r] = e
        th = [threading.Thread(target=drive, args=(r,)) for r in range(nparts)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=600)
        assert all(e is None for e in errs), errs
        for r, c in enumerate(ctxs):
            c.download(locs[r])
    finally:
        for c in ctxs:
            c.close()
    gids = [d.global_ids(r)["cell"][:d.n_owned(r)[0]] for r in range(nparts)]
    return stats.assemble(parts, gids, st.nCells), d.assemble(locs)


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_decomposed_equals_single(x1_2562, nparts, overlap):
    """N loopback subdomains, three steps with the RK3 transport, Kessler and the task: the edge kernel's gather of
    the two scratch columns is exchanged, and the ghosts of what the task wrote are refreshed before the next step
    gathers them"""
    st, ts = state(x1_2562, 26, "moist")

    def fn(c):
        c.set_option("transport", 2)
        c.set_option("microphysics", 1)
        c.set_option("pbl", 1)
        _steps(c, 3)
    key = ("single", "decomposed reference")
    if key not in _ST:
        def single(c):
            fn(c)
            return T.surface_flux_read(c)
        _ST[key] = gpu(st, ts, single)
    ref_acc, ref = _ST[key]
    acc, got = _run_parts(st, ts, nparts, overlap, fn)
    assert np.all(ref_acc["calls"] == 3.0) and np.any(ref_acc["evap"] != 0.0)
    assert same_acc(acc, ref_acc)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def test_keep_check(x1_2562):
    """option keep_check: every keep tail still equals its field after each task of a step with the option
    (graph 0: the tasks of a captured step are not checked), and after the task called directly"""
    st, ts = state(x1_2562, 26, "moist")
    gpu(st, ts, _steps, {"graph": 0, "transport": 2, "microphysics": 1, "pbl": 1, "keep_check": 1})
    gpu(st, ts, one_call, {"keep_check": 1})
    st5, ts5 = state(x1_2562, 5, "mpas0")
    gpu(st5, ts5, one_call, {"keep_check": 1})


def test_option_rules(x1_2562):
    st, ts = state(x1_2562, 5, "mpas0")

    def refused(f, *a):
        with pytest.raises(lib.MpasError) as e:
            f(*a)
        assert EINVAL in str(e.value), str(e.value)
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("pbl") == 0
        ctx.set_option("physics", 2)
        refused(ctx.set_option, "pbl", 1)  # no surface temperature configured
        refused(T.atm_surface_pbl, ctx, DT)
        for bad in (np.nan, np.inf, 0.0, -3.0):
            t = ts.copy()
            t[17] = bad
            refused(T.surface_set_temperature, ctx, t)
        refused(ctx.set_option, "pbl", 1)  # (a refused temperature configures nothing)
        T.surface_set_temperature(ctx, ts)
        for physics in (0, 1):
            ctx.set_option("physics", physics)
            refused(ctx.set_option, "pbl", 1)
            refused(T.atm_surface_pbl, ctx, DT)
        ctx.set_option("physics", 2)
        for bad in (2, -1):
            refused(ctx.set_option, "pbl", bad)
        for bad in (0.0, -720.0, float("nan")):
            refused(T.atm_surface_pbl, ctx, bad)
        ctx.set_option("pbl", 1)
        assert ctx.get_option("pbl") == 1
        refused(ctx.set_option, "forcing", 1)  # both write tend_ru_physics: either order
        assert ctx.get_option("forcing") == 0
        ctx.set_option("pbl", 0)
        ctx.set_option("forcing", 1)
        refused(ctx.set_option, "pbl", 1)
        assert ctx.get_option("pbl") == 0
        ctx.set_option("forcing", 0)
        ctx.set_option("pbl", 1)
        ctx.set_option("physics", 1)  # leaving the MPAS dynamics switches it off
        assert ctx.get_option("pbl") == 0
        ctx.set_option("physics", 2)
        # pbl = 0: a step leaves tend_ru_physics as uploaded, and counts no call
        ctx.upload(st)
        _steps(ctx, 1)
        ctx.sync()
        got = st.copy()
        ctx.download(got, names=["tend_ru_physics"])
        assert np.all(T.surface_flux_read(ctx)["calls"] == 0.0)
    assert np.array_equal(bits(got["tend_ru_physics"]), bits(st["tend_ru_physics"]))


def test_water_budget_of_a_moist_run(x1_2562):
    """The driver's moist JW state at 26 levels, 10 steps of 720 s with the RK3 transport, Kessler and the task: the
    relative drift of sum(area m (qv + qc + qr)) + sum(area (rain - evaporation)) against the drift of the run
    with the transport alone -- the transport's own closure.  The two tasks' own closures are rounding
    (tests/test_kessler.py, tests/test_pbl.py), so ten times the transport's is allowed, floor 1e-13 (the Kessler
    test's convention)."""
    from mpasdyn import moist
    st, ts = state(x1_2562, 26, "moist")
    nC = st.nCells

    def run(c):
        _steps(c, 10)
        return T.precip_read(c), T.surface_flux_read(c)
    w0 = moist.total_water(st)
    (p1, e1), got1 = gpu(st, ts, run, {"transport": 2, "microphysics": 1, "pbl": 1})
    (p0, e0), got0 = gpu(st, ts, run, {"transport": 2})
    d1 = abs(moist.total_water_budget(got1, p1["rain"], e1["evap"]) / w0 - 1.0)
    d0 = abs(moist.total_water_budget(got0, p0["rain"], e0["evap"]) / w0 - 1.0)
    area = 1.0 / st["invAreaCell"][:nC, 0]
    print(f"water budget after 10 steps: drift {d1:.3e} with Kessler and the boundary layer "
          f"({float(np.sum(area * p1['rain']) / np.sum(area)):.4f} mm mean rain, "
          f"{float(np.sum(area * e1['evap']) / np.sum(area)):.4f} mm mean evaporation), {d0:.3e} with the transport alone")
    assert np.all(e0["evap"] == 0.0) and np.all(p0["rain"] == 0.0)
    assert np.sum(p1["rain"]) > 0.0 and np.any(e1["evap"] != 0.0) and np.all(e1["calls"] == 10.0)
    assert np.isfinite(got1["theta_m"]).all()
    assert d1 <= max(10.0 * d0, 1e-13)


def test_task_parity_under_bounds_checks():
    """the task-parity cases in a child pytest on the bounds-checked build (the pattern of
    tests/test_gpu_bounds.py): the kernels touch no memory outside their fields"""
    assert os.path.exists(BOUNDS_LIB), "libmpasdyn_bounds.so missing: run __graft_entry__.build()"
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_task and not bounds", "tests/test_gpu_pbl.py"]
    env = dict(os.environ, MPAS_LIB=BOUNDS_LIB, PYTHONUNBUFFERED="1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "MPAS_EBOUNDS" not in r.stdout, tail
