"""GPU (libmpasdyn k_stats.hip) sigma-level statistics: the task mpas_atm_sigma_stats_accumulate against
its NumPy restatement (tests/stats_ref.py, pinned on the CPU by tests/test_sigma_stats.py), the calls
around it, and option stats_every of mpas_atm_srk3.

Task parity: the sample count n and the ps column bit for bit (no libm call on their path: the bracket is
decided on s = p / ps itself); every other accumulator within the project's per-task bound RTOL_FAST =
1e-11 of its maximum magnitude -- the device's log of s against the host's is the only difference (an
ulp of log s in the weight a, so a few 1e-16 of the interpolated value expected; the observed maximum is
printed and recorded in DESIGN.md §7).  Every registry field stays bit-unchanged.  Everything else here
is bit for bit."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle as O
import stats_ref as R
from helpers import compare_states, make_state
from mpasdyn import decomp, jw, lib, stats
from mpasdyn import mesh as M
from mpasdyn.registry import F_COUNT
from mpasdyn import tasks as T

pytestmark = pytest.mark.gpu

RTOL_FAST = 1e-11
DT = 720.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "mpas-regent_amd", "mpasdyn", "libmpasdyn_bounds.so")
# no bracket at all; one bracket; the smallest column with a choice; LP 8; LP 32; the level-pair layout; level L
# in the last lane
LEVELS = [1, 2, 3, 5, 26, 56, 63]
# one lane's work; fewer targets than LP; more targets than LP below 64 (the lanes loop) and every lane at 64.
# 1.0 lies above nearly every column (s(0) < 1 where the lowest layer has weight), 0.001 below every one
SIGMAS = {1: [0.95], 7: [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, 0.001],
          64: [1.0] + [round(0.95 - 0.015 * i, 3) for i in range(62)] + [0.001]}
# the driver's default levels lie inside every column of the JW state: 1.0 and 0.001 around them go unsampled
JW_SIGMA = [1.0] + list(R.DEFAULT_SIGMA) + [0.001]
EINVAL = "(-1)"

_ST = {}


def state(mesh, L, variant):
    """states built once and never modified: "random" the raw 1-based ids and "mpas0" 0-based ids, both with
    pressures decreasing with the level (stats_ref.decreasing_pressures); "raw" the raw random pressures
    (1-based ids; the columns are not monotone); "jw" the Jablonowski-Williamson state with MPAS-A's initial
    diagnostics, as tests/test_gpu_forcing.py prepares it"""
    key = (L, variant)
    if key not in _ST:
        if variant == "jw":
            st = jw.jw_state(M.zero_based(mesh), L, perturb=True)
            o = O.Oracle(st)
            o.mpas_solve_diagnostics(0, -1)
            o.mpas_reconstruct_2d(False, True)
        elif variant == "raw":
            st = make_state(mesh, L, "random")
        else:
            st = R.decreasing_pressures(make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random").copy())
        _ST[key] = st
    return _ST[key]


def gpu(st, fn, opts=None, sigma=None):
    """fn(ctx) on a fresh physics-2 context holding st, the targets configured first; returns what fn returns
    and the downloaded state"""
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


def one_sample(ctx):
    T.atm_sigma_stats_accumulate(ctx)
    return T.sigma_stats_read(ctx)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in R.STATS + ("ps",)) and set(a) == set(b)


def check_parity(got, ref, label):
    """n and ps bit for bit, the other accumulators within RTOL_FAST of their maximum magnitude"""
    assert np.array_equal(got["n"], ref["n"]), f"{label}: n"
    assert np.array_equal(got["ps"], ref["ps"]), f"{label}: ps"
    worst = 0.0
    for name in R.STATS[1:]:
        assert np.isfinite(ref[name]).all(), name
        scale = float(np.max(np.abs(ref[name])))
        err = float(np.max(np.abs(got[name] - ref[name])))
        if scale == 0.0:  # (nothing sampled: exactly zero)
            assert err == 0.0, f"{label}: {name}"
            continue
        worst = max(worst, err / scale)
        assert err <= RTOL_FAST * scale, f"{label}: {name} off by {err:.3e} = {err / scale:.3e} of its max"
    print(f"{label}: max|gpu - restatement| over the accumulators = {worst:.3e} of the accumulator's max")


def check_sampling(hit, L):
    """every case holds sampled and unsampled pairs, at least half of them sampled (one level: none at all)"""
    if L == 1:
        assert not hit.any()
    else:
        assert 0.5 <= hit.mean() < 1.0, hit.mean()


def parity_case(st, sigma, label):
    ref = R.new_acc(st.nCells, len(sigma))
    check_sampling(R.accumulate(ref, st, sigma)["hit"], st.L)
    acc, got = gpu(st, one_sample, sigma=sigma)
    check_parity(acc, ref, label)
    bad = compare_states(got, st, rtol=0.0)  # the task writes no field
    assert not bad, bad[:6]
    return acc


@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("ns", sorted(SIGMAS))
@pytest.mark.parametrize("L", LEVELS)
def test_task(x1_2562, L, ns, variant):
    acc = parity_case(state(x1_2562, L, variant), SIGMAS[ns], f"L={L} nsigma={ns} {variant}")
    if L == 1:  # no bracket exists: everything stays 0 but the ps column
        assert all(not acc[name].any() for name in R.STATS) and np.all(acc["ps"][:, 2] == 1.0)


@pytest.mark.parametrize("ns", [7, 64])
@pytest.mark.parametrize("L", [26, 56])
def test_task_on_raw_random_pressures(x1_2562, L, ns):
    """columns that are not monotone: the lowest qualifying bracket, the same on device and host"""
    st = state(x1_2562, L, "raw")
    s = R.columns(st)["s"]
    assert np.mean(np.any(np.diff(s, axis=1) > 0.0, axis=1)) > 0.9
    parity_case(st, SIGMAS[ns], f"L={L} nsigma={ns} raw pressures")


@pytest.mark.parametrize("L", [26, 56])
def test_task_on_the_jw_state(x1_2562, L):
    parity_case(state(x1_2562, L, "jw"), JW_SIGMA, f"L={L} jw")


def test_reset_and_configure_again(x1_2562):
    st = state(x1_2562, 26, "mpas0")

    def fn(ctx):
        assert ctx.get_option("stats_samples") == 0
        a = one_sample(ctx)
        assert ctx.get_option("stats_samples") == 1 and a["n"].any()
        T.sigma_stats_reset(ctx)
        z = T.sigma_stats_read(ctx)
        assert all(not z[k].any() for k in z) and ctx.get_option("stats_samples") == 0
        b = one_sample(ctx)  # from zero again: the same bits
        assert same_bits(a, b)
        T.sigma_stats_configure(ctx, SIGMAS[64])  # another nsigma: new, zeroed accumulators
        z = T.sigma_stats_read(ctx)
        assert z["n"].shape == (st.nCells, 64) and all(not z[k].any() for k in z)
        return one_sample(ctx)
    acc, _ = gpu(st, fn, sigma=SIGMAS[7])
    ref = R.new_acc(st.nCells, 64)
    R.accumulate(ref, st, SIGMAS[64])
    check_parity(acc, ref, "configured again with 64 targets")


def test_two_calls_on_two_states(x1_2562):
    a, b = state(x1_2562, 26, "mpas0"), state(x1_2562, 26, "jw")
    sigma = list(R.DEFAULT_SIGMA)

    def fn(ctx):
        T.atm_sigma_stats_accumulate(ctx)
        ctx.upload(b)
        return one_sample(ctx)
    acc, _ = gpu(a, fn, sigma=sigma)
    ref = R.new_acc(a.nCells, len(sigma))
    R.accumulate(ref, a, sigma)
    R.accumulate(ref, b, sigma)
    assert np.all(ref["ps"][:, 2] == 2.0) and ref["n"].max() == 2.0
    check_parity(acc, ref, "two states")


def _steps(ctx, n):
    for _ in range(n):
        T.atm_srk3(ctx, DT, 1)


@pytest.mark.parametrize("forcing", [0, 1])
def test_step_option_is_the_composition(x1_2562, forcing):
    """four steps with stats_every = 2 == the same steps without the option and the task called by hand after
    the second and the fourth: bit for bit in the accumulators and in every field"""
    st = state(x1_2562, 26, "jw")
    sigma = list(R.DEFAULT_SIGMA)

    def with_option(ctx):
        ctx.set_option("stats_every", 2)
        _steps(ctx, 4)
        assert ctx.get_option("stats_samples") == 2
        return T.sigma_stats_read(ctx)

    def by_hand(ctx):
        for _ in range(2):
            _steps(ctx, 2)
            T.atm_sigma_stats_accumulate(ctx)
        return T.sigma_stats_read(ctx)
    acc, got = gpu(st, with_option, {"forcing": forcing}, sigma)
    ref_acc, ref = gpu(st, by_hand, {"forcing": forcing}, sigma)
    assert np.all(acc["ps"][:, 2] == 2.0) and acc["n"].max() == 2.0 and np.isfinite(acc["TT"]).all()
    assert same_bits(acc, ref_acc)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    assert not np.array_equal(got["theta_m"], st["theta_m"])


def test_graph_on_equals_graph_off(x1_2562):
    """the sample is launched behind the replayed step, in no captured graph: graph_captures is what it is
    without the option"""
    st = state(x1_2562, 26, "jw")
    sigma = list(R.DEFAULT_SIGMA)
    out = {}
    for graph, every in ((0, 1), (1, 1), (1, 0)):
        def fn(ctx):
            ctx.set_option("stats_every", every)
            _steps(ctx, 3)
            ctx.sync()
            return T.sigma_stats_read(ctx), ctx.get_option("graph_captures"), ctx.get_option("stats_samples")
        out[graph, every] = gpu(st, fn, {"graph": graph, "forcing": 1}, sigma)
    (acc0, cap0, n0), got0 = out[0, 1]
    (acc1, cap1, n1), got1 = out[1, 1]
    (accn, capn, nn), gotn = out[1, 0]
    assert (cap0, n0) == (0, 3) and n1 == 3 and nn == 0 and cap1 == capn >= 1
    assert same_bits(acc0, acc1) and acc1["n"].max() == 3.0 and not accn["n"].any()
    for other in (got0, gotn):
        bad = compare_states(got1, other, rtol=0.0)
        assert not bad, bad[:6]


@pytest.mark.parametrize("name", ["L5;physics=2", "L56;physics=2,forcing=1"])
def test_rows_without_the_option_are_the_recorded_ones(name):
    """stats_every = 0, the targets configured: the step's timing rows are those recorded before the feature
    (tests/golden/srk3_rows_x1.2562.json); with the option on, one more row"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import record_step_rows as RS
    with open(RS.FIXTURE) as f:
        want = RS.unpack_steps(json.load(f), name)
    L, opts, dt, schedule, _dec = RS.CONFIGS[name]
    st = RS._state(L, True)
    with lib.Context(*st.dims()) as ctx:
        RS._set_all(ctx, opts)
        T.sigma_stats_configure(ctx, SIGMAS[7])
        ctx.set_option("stats_every", 0)
        ctx.upload(st)
        ctx.timing(True)
        got = RS._four_steps(ctx, dt, schedule)
        ctx.set_option("stats_every", 1)
        more = RS._four_steps(ctx, dt, schedule)
    assert got == want
    assert all(["atm_sigma_stats_accumulate", 1] in rows for rows in more)
    assert all(len(m) == len(w) + 1 for m, w in zip(more, want))


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
                parts[r] = T.sigma_stats_read(ctxs[r], d.n_owned(r)[0])
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
    st = state(x1_2562, 26, "jw")
    sigma = list(R.DEFAULT_SIGMA)

    def fn(c):
        c.set_option("physics", 2)
        c.set_option("forcing", 1)
        T.sigma_stats_configure(c, sigma)
        c.set_option("stats_every", 1)
        _steps(c, 2)
    key = ("single", "decomposed reference")
    if key not in _ST:
        def single(c):
            fn(c)
            return T.sigma_stats_read(c)
        _ST[key] = gpu(st, single)
    ref_acc, ref = _ST[key]
    acc, got = _run_parts(st, nparts, overlap, fn)
    assert ref_acc["n"].max() == 2.0
    assert same_bits(acc, ref_acc)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    nC = st.nCells
    lat, area = st["lat"][:nC, 0], 1.0 / st["invAreaCell"][:nC, 0]
    za, zb = stats.zonal_means(acc, lat, area, 36), stats.zonal_means(ref_acc, lat, area, 36)
    assert all(np.array_equal(za[k], zb[k], equal_nan=True) for k in zb) and np.isfinite(zb["u"]).any()


def test_error_codes(x1_2562):
    st = state(x1_2562, 5, "mpas0")
    with lib.Context(*st.dims()) as ctx:
        def refused(fn, *a):
            with pytest.raises(lib.MpasError) as e:
                fn(*a)
            assert EINVAL in str(e.value), str(e.value)
        assert ctx.get_option("stats_every") == 0 and ctx.get_option("stats_samples") == 0
        ctx.set_option("physics", 2)
        refused(T.atm_sigma_stats_accumulate, ctx)       # not configured
        refused(ctx.set_option, "stats_every", 1)        # no configured list
        refused(T.sigma_stats_reset, ctx)
        for bad in ([1.1, 0.5], [0.5, 0.0], [0.5, -0.1], [0.5, 0.5], [0.4, 0.5], [float("nan")],
                    list(np.linspace(0.99, 0.01, 65))):  # outside (0, 1]; not strictly decreasing; 65 targets
            refused(T.sigma_stats_configure, ctx, bad)
        assert ctx.lib.mpas_sigma_stats_configure(ctx.h, -1, None) == -1
        T.sigma_stats_configure(ctx, [1.0, 0.5])
        out = np.zeros((st.nCells, 3))
        for stat in (-1, 10):
            assert ctx.lib.mpas_sigma_stats_read(ctx.h, stat, out.ctypes.data, out.strides[0], out.strides[1]) == -1
        refused(ctx.set_option, "stats_every", -1)
        ctx.set_option("stats_every", 3)
        assert ctx.get_option("stats_every") == 3
        ctx.set_option("physics", 1)                     # leaving the MPAS dynamics switches it off
        assert ctx.get_option("stats_every") == 0
        refused(T.atm_sigma_stats_accumulate, ctx)       # physics != 2
        refused(ctx.set_option, "stats_every", 1)
        ctx.set_option("physics", 2)
        ctx.set_option("stats_every", 1)
        T.sigma_stats_configure(ctx, [])                 # freed: the option goes with the list
        assert ctx.get_option("stats_every") == 0
        refused(T.atm_sigma_stats_accumulate, ctx)
        assert lib.load().mpas_field_count() == F_COUNT  # no field id moved


def test_keep_check_step_with_the_option(x1_2562):
    """option keep_check: every keep tail still equals its field after each task of a sampled step (graph 0:
    the tasks of a captured step are not checked)"""
    st = state(x1_2562, 26, "jw")

    def fn(ctx):
        ctx.set_option("stats_every", 1)
        _steps(ctx, 1)
        return ctx.get_option("stats_samples")
    n, _ = gpu(st, fn, {"graph": 0, "forcing": 1, "keep_check": 1}, list(R.DEFAULT_SIGMA))
    assert n == 1


def test_task_parity_under_bounds_checks():
    """the task-parity cases in a child pytest on the bounds-checked build (the pattern of
    tests/test_gpu_forcing.py): the kernel touches no field outside its rows"""
    assert os.path.exists(BOUNDS_LIB), "libmpasdyn_bounds.so missing: run __graft_entry__.build()"
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_task and not bounds", "tests/test_gpu_sigma_stats.py"]
    env = dict(os.environ, MPAS_LIB=BOUNDS_LIB, PYTHONUNBUFFERED="1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "MPAS_EBOUNDS" not in r.stdout, tail
