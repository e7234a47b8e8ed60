"""GPU (libmpasdyn k_kessler.hip) Kessler warm-rain microphysics: the task mpas_atm_kessler_microphysics against its
NumPy restatement (tests/kessler_ref.py, pinned on the CPU by tests/test_kessler.py), its precipitation
accumulators, and option microphysics = 1 of mpas_atm_srk3.

Task parity: every written field -- theta_m, rtheta_p, exner, pressure_p, rt_diabatic_tend, and qv, qc, qr each on
its own -- within the project's per-task bound RTOL_FAST = 1e-11 of that field's largest magnitude; the device's
pow / exp / log against the host's are the only differences.  The subcycle count n = ceil(x) enters as an integer:
a column whose x lies within 1e-9 relative of an integer >= 1 is left out (at most 0.5 % of a case's columns, else
the case fails; with the generator's seed the restatement leaves out none, tests/test_kessler.py).  The call
counter is bit for bit, the two rain accumulators within the same bound; dry columns are bit for bit; every field
the task does not write is bit-unchanged, as are scalars 3..7, level L and the zero slot of what it writes.  The
observed maxima are printed and recorded in DESIGN.md §7.  Everything else here is bit for bit."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import kessler_ref as K
import oracle as O
from helpers import compare_states, make_state
from mpasdyn import decomp, jw, lib, stats
from mpasdyn import mesh as M
from mpasdyn import tasks as T

pytestmark = pytest.mark.gpu

RTOL_FAST = 1e-11
DT = 720.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "mpas-regent_amd", "mpasdyn", "libmpasdyn_bounds.so")
# one level; the first shuffle; the smallest column with an interior level; LP 8 with eight columns per wavefront;
# LP 32 with two; the benchmark's L (the level-pair layout); level L in the last lane
LEVELS = [1, 2, 3, 5, 26, 56, 63]
EINVAL = "(-1)"
ACC = ("rain", "rain_last", "calls")

_ST = {}


def state(mesh, L, variant):
    """states built once and never modified: "random" (raw 1-based ids) and "mpas0" (0-based ids) carry the
    generator's physical columns; "moist" is the driver's moist Jablonowski-Williamson state with MPAS-A's initial
    diagnostics, qc = 2e-3 and qr = 1e-3 put below 3 km (and in the lowest level) so that it rains"""
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
        else:
            st = K.physical_columns(make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random"))
        _ST[key] = st
    return _ST[key]


def gpu(st, fn, opts=None, sigma=None):
    """fn(ctx) on a fresh physics-2 context holding st; returns what fn returns and the downloaded state"""
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        if os.environ.get("MPAS_LIB") == BOUNDS_LIB:  # (the child run of the bounds test)
            assert ctx.get_option("bounds") == 1, "not the bounds-checked build"
        ctx.set_option("physics", 2)
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


def same_acc(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ACC) and set(a) == set(b) == set(ACC)


def one_call(ctx):
    T.atm_kessler_microphysics(ctx, DT)
    return T.precip_read(ctx)


def _steps(c, n=1):
    for _ in range(n):
        T.atm_srk3(c, DT, 1)


@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("L", LEVELS)
def test_task(x1_2562, L, variant):
    st = state(x1_2562, L, variant)
    nC = st.nCells
    ref, racc = st.copy(), K.new_acc(nC)
    d = K.kessler(ref, DT, racc)
    acc, got = gpu(st, one_call)
    out = K.near_integer(d["x"])
    assert out.sum() <= 0.005 * nC, f"{int(out.sum())} columns with x within 1e-9 of an integer"
    keep = ~out
    worst = {}

    def close(name, g, r):
        assert np.isfinite(r).all(), name
        scale = float(np.max(np.abs(r)))
        err = float(np.max(np.abs(g - r)))
        worst[name] = err / scale if scale else err
        assert scale > 0.0 and err <= RTOL_FAST * scale, f"{name} off by {err:.3e} = {err / scale:.3e} of its max"
    for name in ("theta_m", "rtheta_p", "exner", "pressure_p", "rt_diabatic_tend"):
        close(name, got[name][:nC, :L][keep], ref[name][:nC, :L][keep])
    for i, name in enumerate(("qv", "qc", "qr")):
        close(name, got["scalars"][:nC, :L, i][keep], ref["scalars"][:nC, :L, i][keep])
    assert np.array_equal(acc["calls"], racc["calls"]) and np.all(acc["calls"] == 1.0)
    close("rain", acc["rain"][keep], racc["rain"][keep])
    close("rain_last", acc["rain_last"][keep], racc["rain_last"][keep])
    assert np.array_equal(bits(acc["rain"]), bits(acc["rain_last"]))  # (the first call: 0.0 + P)
    print(f"L={L} {variant}: n in [{d['n'].min()}, {d['n'].max()}], {int(out.sum())} columns left out; "
          "max|gpu - restatement| / max|field|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # the task did something, and the restatement agrees on where it did nothing
    assert np.any(ref["rt_diabatic_tend"][:nC, :L] != 0.0) and np.any(racc["rain"] > 0.0)
    # dry columns: bit for bit, as on the CPU
    dry = K.DRY(nC)
    for name in ("theta_m", "rtheta_p"):
        assert np.array_equal(bits(got[name][:nC, :L][dry]), bits(st[name][:nC, :L][dry])), name
    assert np.array_equal(bits(got["scalars"][:nC, :L, :3][dry]), bits(st["scalars"][:nC, :L, :3][dry]))
    assert np.all(bits(got["rt_diabatic_tend"][:nC, :L][dry]) == 0) and np.all(bits(acc["rain"][dry]) == 0)
    # nothing else is written: every other field, scalars 3..7, and level L and the zero slot of the outputs
    bad = compare_states(got, st, rtol=0.0, skip=set(K.WRITTEN))
    assert not bad, bad[:6]
    assert np.array_equal(bits(got["scalars"][..., 3:]), bits(st["scalars"][..., 3:]))
    for name in K.WRITTEN:
        assert np.array_equal(bits(got[name][:, L]), bits(st[name][:, L])), name
        assert np.array_equal(bits(got[name][nC]), bits(st[name][nC])), name


def test_rain_a_rounding_below_zero(x1_2562):
    """a rain the transport's limiter left a rounding below zero: no NaN on the device either, and the same parity"""
    st = state(x1_2562, 5, "mpas0").copy()
    nC, L = st.nCells, st.L
    st["scalars"][:nC:2, 0, 2] = -1e-20
    st["scalars"][1:nC:4, 3, 2] = -3e-19
    ref, racc = st.copy(), K.new_acc(nC)
    d = K.kessler(ref, DT, racc)
    acc, got = gpu(st, one_call)
    assert not K.near_integer(d["x"]).any()
    for name in K.WRITTEN:
        assert np.isfinite(got[name]).all(), name
        g, r = (x[name][:nC, :L, :3] if name == "scalars" else x[name][:nC, :L] for x in (got, ref))
        assert float(np.max(np.abs(g - r))) <= RTOL_FAST * float(np.max(np.abs(r))), name
    assert np.isfinite(acc["rain"]).all()
    assert float(np.max(np.abs(acc["rain"] - racc["rain"]))) <= RTOL_FAST * float(np.max(racc["rain"]))
    assert got["scalars"][:nC, :L, :3].min() >= 0.0


def test_two_calls_add(x1_2562):
    st = state(x1_2562, 26, "mpas0")

    def fn(c):
        a = one_call(c)
        b = one_call(c)
        T.precip_reset(c)
        return a, b, T.precip_read(c)
    (a, b, z), _ = gpu(st, fn)
    assert np.any(a["rain_last"] > 0.0) and np.any(b["rain_last"] != a["rain_last"])
    assert np.array_equal(bits(b["rain"]), bits(a["rain_last"] + b["rain_last"]))
    assert np.all(a["calls"] == 1.0) and np.all(b["calls"] == 2.0)
    assert all(np.all(bits(z[k]) == 0) for k in ACC)


@pytest.mark.parametrize("transport", [2, 0])
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("L", [5, 56])
def test_step_is_the_composition(x1_2562, L, exact, transport):
    """atm_srk3 with microphysics = 1 == atm_srk3 with microphysics = 0, then the task: bit for bit in every field
    and accumulator"""
    st = state(x1_2562, L, "moist")
    opts = {"exact": exact, "transport": transport}

    def step(c):
        _steps(c)
        return T.precip_read(c)

    def composed(c):
        _steps(c)
        return one_call(c)
    acc, got = gpu(st, step, dict(opts, microphysics=1))
    racc, ref = gpu(st, composed, dict(opts, microphysics=0))
    assert np.any(acc["rain"] > 0.0) and np.all(acc["calls"] == 1.0)
    assert np.any(got["rt_diabatic_tend"] != 0.0)
    assert same_acc(acc, racc)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def test_step_sample_sees_the_adjusted_state(x1_2562):
    """with stats_every = 1 the step's sample comes after the task"""
    st = state(x1_2562, 26, "moist")
    sigma = list(stats.DEFAULT_SIGMA)

    def step(c):
        _steps(c)
        return T.sigma_stats_read(c)

    def composed(c):
        _steps(c)
        T.atm_kessler_microphysics(c, DT)
        T.atm_sigma_stats_accumulate(c)
        return T.sigma_stats_read(c)
    a, got = gpu(st, step, {"transport": 2, "microphysics": 1, "stats_every": 1}, sigma=sigma)
    b, ref = gpu(st, composed, {"transport": 2}, sigma=sigma)
    c, _ = gpu(st, step, {"transport": 2, "stats_every": 1}, sigma=sigma)
    assert a["n"].max() == 1.0 and set(a) == set(b)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
    assert not np.array_equal(a["T"], c["T"])  # (the sample of the unadjusted state differs)
    assert not compare_states(got, ref, rtol=0.0)


def test_graph_replay_and_recapture(x1_2562):
    st = state(x1_2562, 26, "moist")
    out, accs = {}, {}
    for graph in (0, 1):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("graph", graph)
            ctx.set_option("physics", 2)
            ctx.set_option("transport", 2)
            ctx.set_option("microphysics", 1)
            ctx.upload(st)
            _steps(ctx, 2)
            ctx.sync()
            assert ctx.get_option("graph_captures") == graph
            assert ctx.get_option("graph_launches") == 2 * graph
            ctx.download(got)
            accs[graph] = T.precip_read(ctx)
            if graph:
                ctx.set_option("microphysics", 0)  # toggling the option: a new capture
                _steps(ctx, 1)
                ctx.sync()
                assert ctx.get_option("graph_captures") == 2
                assert np.all(T.precip_read(ctx)["calls"] == 2.0)  # (no task in that step)
                ctx.set_option("microphysics", 1)
                ctx.timing(True)  # the task appears in the per-task timing, once per step
                _steps(ctx, 1)
                ctx.sync()
                rep = ctx.timing_report()
                assert rep["atm_kessler_microphysics"][0] == 1, rep
        out[graph] = got
    assert np.all(accs[1]["calls"] == 2.0) and np.any(accs[1]["rain"] > 0.0)
    assert same_acc(accs[1], accs[0])
    bad = compare_states(out[1], out[0], rtol=0.0)
    assert not bad, bad[:6]


def _run_parts(st, nparts, overlap, fn):
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
        lib.halo_loopback(ctxs)

        def drive(r):
            try:
                fn(ctxs[r])
                ctxs[r].sync()
                parts[r] = T.precip_read(ctxs[r], d.n_owned(r)[0])
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
    """N loopback subdomains, three steps with the RK3 transport and the task: the ghosts of what the task wrote
    are refreshed before the next step gathers them"""
    st = state(x1_2562, 26, "moist")

    def fn(c):
        c.set_option("physics", 2)
        c.set_option("transport", 2)
        c.set_option("microphysics", 1)
        _steps(c, 3)
    key = ("single", "decomposed reference")
    if key not in _ST:
        def single(c):
            fn(c)
            return T.precip_read(c)
        _ST[key] = gpu(st, single)
    ref_acc, ref = _ST[key]
    acc, got = _run_parts(st, nparts, overlap, fn)
    assert np.all(ref_acc["calls"] == 3.0) and np.any(ref_acc["rain"] > 0.0)
    assert same_acc(acc, ref_acc)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def test_keep_check(x1_2562):
    """option keep_check: every keep tail still equals its field after each task of a step with the option
    (graph 0: the tasks of a captured step are not checked), and after the task called directly"""
    st = state(x1_2562, 26, "moist")
    gpu(st, _steps, {"graph": 0, "transport": 2, "microphysics": 1, "keep_check": 1})
    gpu(st, one_call, {"keep_check": 1})
    gpu(state(x1_2562, 5, "mpas0"), one_call, {"keep_check": 1})


def test_option_rules(x1_2562):
    st = state(x1_2562, 5, "mpas0")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("microphysics") == 0
        for physics in (0, 1):
            ctx.set_option("physics", physics)
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("microphysics", 1)
            assert EINVAL in str(e.value)
            with pytest.raises(lib.MpasError) as e:
                T.atm_kessler_microphysics(ctx, DT)
            assert EINVAL in str(e.value)
        ctx.set_option("physics", 2)
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("microphysics", bad)
            assert EINVAL in str(e.value)
        ctx.set_option("microphysics", 1)
        assert ctx.get_option("microphysics") == 1
        ctx.set_option("physics", 1)  # leaving the MPAS dynamics switches it off
        assert ctx.get_option("microphysics") == 0
        ctx.set_option("physics", 2)
        # microphysics = 0: a step leaves rt_diabatic_tend as uploaded, and counts no call
        ctx.upload(st)
        _steps(ctx, 1)
        ctx.sync()
        got = st.copy()
        ctx.download(got, names=["rt_diabatic_tend"])
        assert np.all(T.precip_read(ctx)["calls"] == 0.0)
    assert np.array_equal(bits(got["rt_diabatic_tend"]), bits(st["rt_diabatic_tend"]))


def test_water_budget_of_a_moist_run(x1_2562):
    """The driver's moist JW state at 26 levels, 10 steps of 720 s with the RK3 transport: the relative drift of
    sum(area m (qv + qc + qr)) + sum(area rain) with the task, against the drift of the same run without it --
    the transport's own closure.  The task's own closure is rounding (tests/test_kessler.py), so ten times the
    transport's is allowed, floor 1e-13."""
    st = state(x1_2562, 26, "moist")
    nC = st.nCells
    area = 1.0 / st["invAreaCell"][:nC, 0]

    def total(s, rain):
        return float(np.sum(area * K.water(s)) + np.sum(area * rain))

    def run(c):
        _steps(c, 10)
        return T.precip_read(c)
    w0 = total(st, np.zeros(nC))
    acc1, got1 = gpu(st, run, {"transport": 2, "microphysics": 1})
    acc0, got0 = gpu(st, run, {"transport": 2, "microphysics": 0})
    d1 = abs(total(got1, acc1["rain"]) / w0 - 1.0)
    d0 = abs(total(got0, acc0["rain"]) / w0 - 1.0)
    print(f"water budget after 10 steps: drift {d1:.3e} with the task ({float(np.sum(area * acc1['rain']) / np.sum(area)):.4f} "
          f"mm mean rain), {d0:.3e} without (the transport's closure)")
    assert np.all(acc0["rain"] == 0.0) and np.sum(acc1["rain"]) > 0.0 and np.all(acc1["calls"] == 10.0)
    assert np.isfinite(got1["theta_m"]).all()
    assert not np.array_equal(got0["scalars"][:nC, :26, 0], st["scalars"][:nC, :26, 0])  # (the transport moved qv)
    assert d1 <= max(10.0 * d0, 1e-13)


def test_task_parity_under_bounds_checks():
    """the task-parity cases in a child pytest on the bounds-checked build (the pattern of
    tests/test_gpu_bounds.py): the kernel touches no memory outside its fields"""
    assert os.path.exists(BOUNDS_LIB), "libmpasdyn_bounds.so missing: run __graft_entry__.build()"
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_task and not bounds", "tests/test_gpu_kessler.py"]
    env = dict(os.environ, MPAS_LIB=BOUNDS_LIB, PYTHONUNBUFFERED="1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "MPAS_EBOUNDS" not in r.stdout, tail
