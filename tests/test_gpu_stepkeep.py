"""Option `stepkeep` (tests/test_stepkeep_identity.py is the CPU premise).

In the reference semantics no task of atm_srk3 writes u, ru, rw, rho_zz, theta_m, rho_p, rtheta_p, h, zz, exner
or the base fields, so from the second consecutive step on (generation >= 1) the step runs no solve_diagnostics
launch and its setup launch stores w_2 and vert_imp's columns alone; with stepkeep = 2, from the third on
(generation 2), stage 0's dyn_tend does not run either (its w is restored from a copy) and stage 2 forms
tend_u, v and w alone.  Every field keeps its bits against stepkeep = 0, the parent's step; every call from
outside that could change a field or the form of the step sends the generation back to 0; where the step
is not the headline's (hfuse, exact, the reference driver's schedule, the MPAS forms, a decomposed context)
the generation stays 0.  The small mesh runs with hfuse = 0: its default, the combined launches, is one of
the inactive paths.
"""
import os
import sys

import numpy as np
import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 720.0
SOLVE = "atm_compute_solve_diagnostics"
DYN0 = "atm_compute_dyn_tend_work[rk0"


def _run(st, opts, script, exact=0):
    """script: a list of callables fn(ctx), or "step" / ("step", dt, schedule); returns the state after every
    step and the generation read after every step"""
    snaps, gens = [], []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("exact", exact)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload(st)
        for item in script:
            if item == "step" or (isinstance(item, tuple) and item[0] == "step"):
                dt, schedule = (DT, 1) if item == "step" else item[1:]
                T.atm_srk3(ctx, dt, schedule)
                gens.append(ctx.get_option("stepkeep_gen"))
                ctx.sync()
                got = st.copy()
                ctx.download(got)
                snaps.append(got)
            else:
                item(ctx)
    return snaps, gens


def _same(on, off, what=""):
    assert len(on) == len(off)
    for n, (a, b) in enumerate(zip(on, off)):
        bad = compare_states(a, b, rtol=0.0)
        assert not bad, f"{what} after step {n + 1}: {bad[:6]}"


_OFF = {}


def _off5(mesh, L, variant, graph):
    """five steps of the parent's step (stepkeep 0): computed once per case, never modified"""
    key = (L, variant, graph)
    if key not in _OFF:
        _OFF[key] = _run(_state(mesh, L, variant), dict(hfuse=0, graph=graph, stepkeep=0), ["step"] * 5)[0]
    return _OFF[key]


@pytest.mark.parametrize("stepkeep", [1, 2])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 56])
def test_stepkeep_bit_identical(x1_2562, L, variant, graph, stepkeep):
    """stepkeep against 0: every field after each of five consecutive steps; the generation reads 1, 2, 2, ..."""
    st = _state(x1_2562, L, variant)
    keep_check = 1 if (graph == 0 and L == 56 and variant == "random") else 0  # (eager launches, once per value)
    on, gens = _run(st, dict(hfuse=0, graph=graph, stepkeep=stepkeep, keep_check=keep_check), ["step"] * 5)
    assert gens == [1, 2, 2, 2, 2]
    _same(on, _off5(x1_2562, L, variant, graph))


@pytest.mark.parametrize("stepkeep", [1, 2])
def test_stepkeep_timing_rows(x1_2562, stepkeep):
    """under per-task timing step 1 has the solve_diagnostics and the stage-0 dyn_tend rows; step 3 has no
    solve_diagnostics row and, with stepkeep = 2, no stage-0 dyn_tend row but the restore of w; bench.py's
    table takes every key"""
    sys.path.insert(0, REPO)
    import bench
    st = _state(x1_2562, 5, "random")
    reps = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.set_option("stepkeep", stepkeep)
        ctx.upload(st)
        ctx.timing(True)
        for _ in range(3):
            ctx.timing_reset()
            T.atm_srk3(ctx, DT, 1)
            ctx.sync()
            reps.append(ctx.timing_report())
    live = [{k for k, (calls, _) in r.items() if calls} for r in reps]
    assert sum(k.startswith(SOLVE) for k in live[0]) == 2 and sum(k.startswith(DYN0) for k in live[0]) == 1
    assert not any(k.startswith(SOLVE) for k in live[1]) and sum(k.startswith(DYN0) for k in live[1]) == 1
    assert not any(k.startswith(SOLVE) for k in live[2])
    if stepkeep == 2:
        assert "stepkeep_save_w" in live[1] and "stepkeep_save_w" not in live[0] | live[2]
        assert not any(k.startswith(DYN0) for k in live[2]) and "stepkeep_restore_w" in live[2]
        assert "atm_compute_dyn_tend_work[rk>0+v-A]" in live[2], sorted(live[2])
    else:
        assert live[2] == live[1] and sum(k.startswith(DYN0) for k in live[2]) == 1
        assert not any(k.startswith("stepkeep_") for k in live[0] | live[1] | live[2])
    for r, names in zip(reps, live):
        t = bench.task_table({k: r[k] for k in names}, st.dims(), 1, physics=0, ddx=True)
        assert t["atm_compute_dyn_tend_work"]["launches_per_step"] == sum(
            k.startswith("atm_compute_dyn_tend_work") for k in names)


@pytest.mark.parametrize("stepkeep", [1, 2])
def test_stepkeep_graph_counts(x1_2562, stepkeep):
    """one capture per generation whose launches differ -- at most three per (dt, schedule) -- then replays"""
    st = _state(x1_2562, 5, "random")
    per = 2 if stepkeep == 1 else 3
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.set_option("stepkeep", stepkeep)
        ctx.upload(st)
        n = 0
        for dt, steps, caps in ((720.0, 6, per), (360.0, 4, 2 * per), (720.0, 4, 2 * per), (360.0, 1, 2 * per)):
            for _ in range(steps):
                T.atm_srk3(ctx, dt, 1)
            n += steps
            ctx.sync()
            assert ctx.get_option("graph_captures") == caps, (dt, steps)
            assert ctx.get_option("graph_launches") == n


def _upload(name):
    def fn(ctx, other):
        ctx.upload(other, names=[name])
    return fn


def _toggle(name, other_value):
    """the option to another value, a step, the option back"""
    def fn(ctx, other):
        orig = ctx.get_option(name)
        ctx.set_option(name, other_value)
        T.atm_srk3(ctx, DT, 1)
        ctx.set_option(name, orig)
    return fn


def _timing(ctx, other):
    ctx.timing(True)
    T.atm_srk3(ctx, DT, 1)
    ctx.timing(False)


CHANGES = {
    **{"upload_" + n: _upload(n) for n in ("u", "ru", "theta_m", "w", "rho_zz", "v", "divergence")},
    "fill": lambda ctx, other: ctx.fill_synthetic(4242),
    "solve_diagnostics": lambda ctx, other: T.atm_compute_solve_diagnostics(ctx, False, 0),
    "integration_setup": lambda ctx, other: T.atm_rk_integration_setup(ctx),
    "core_init": lambda ctx, other: T.atm_core_init(ctx),
    "stepkeep": _toggle("stepkeep", 0),
    "ntu": _toggle("ntu", 0),
    "physics": _toggle("physics", 1),
    "timing": _timing,
}


@pytest.mark.parametrize("stepkeep", [1, 2])
@pytest.mark.parametrize("change", sorted(CHANGES))
def test_stepkeep_invalidation(x1_2562, change, stepkeep):
    """three steps, a call from outside, three steps: every field after every step equals the stepkeep 0 twin
    given the same calls; but for switching the timing, the generation is 0 right after the call"""
    L = 26
    st = mpas_state(x1_2562, L, "mpas0") if change == "physics" else _state(x1_2562, L, "random")
    other = make_state(x1_2562, L, "random", seed=77)
    gen_after = []

    def act(ctx):
        CHANGES[change](ctx, other)
        gen_after.append(ctx.get_option("stepkeep_gen"))
    script = ["step"] * 3 + [act] + ["step"] * 3
    on, gens = _run(st, dict(hfuse=0, stepkeep=stepkeep), script)
    if change == "timing":  # (the eager step takes the same decisions: the generation goes on)
        assert gen_after == [2] and gens == [1, 2, 2, 2, 2, 2]
    else:
        assert gen_after == [0] and gens == [1, 2, 2, 1, 2, 2]
    gen_after.clear()
    off, gens0 = _run(st, dict(hfuse=0, stepkeep=0), script)
    assert gens0 == [0] * 6
    _same(on, off, change)
    if change in ("upload_u", "upload_ru", "upload_theta_m", "upload_rho_zz", "fill"):
        # ... and the new values reached the step: without them it ends elsewhere (w below level L and the
        # diagnostics are formed again by the steps, so a new w, v or divergence need not show three steps on)
        plain = _run(st, dict(hfuse=0, stepkeep=0), ["step"] * 6)[0]
        assert compare_states(plain[5], off[5], rtol=0.0)


@pytest.mark.parametrize("stepkeep", [1, 2])
def test_stepkeep_dt_and_schedule(x1_2562, stepkeep):
    """another dt or schedule starts from generation 0 (the coefficients and the launches depend on both); the
    reference driver's schedule runs stage 0 at rk_step > 0: inactive; download and sync reset nothing"""
    st = _state(x1_2562, 26, "random")
    snap = st.copy()
    script = (["step"] * 3 + [("step", 360.0, 1)] * 3 + [("step", 720.0, 0)] * 2 + ["step"] * 2 +
              [lambda ctx: ctx.sync(), lambda ctx: ctx.download(snap)] + ["step"])
    on, gens = _run(st, dict(hfuse=0, stepkeep=stepkeep), script)
    assert gens == [1, 2, 2, 1, 2, 2, 0, 0, 1, 2, 2]
    off, _ = _run(st, dict(hfuse=0, stepkeep=0), script)
    _same(on, off)


@pytest.mark.parametrize("stepkeep", [1, 2])
@pytest.mark.parametrize("path", ["hfuse", "exact", "schedule0", "physics1", "physics2", "tmedge"])
def test_stepkeep_inactive_paths(x1_2562, path, stepkeep):
    """where the step is not the headline's the generation stays 0 and the fields are the stepkeep 0 run's"""
    mpas = path.startswith("physics")
    st = mpas_state(x1_2562, 5, "mpas0") if mpas else _state(x1_2562, 5, "random")
    opts = {"hfuse": dict(hfuse=1), "exact": dict(hfuse=0), "schedule0": dict(hfuse=0), "physics1": dict(hfuse=0, physics=1),
            "physics2": dict(hfuse=0, physics=2), "tmedge": dict(hfuse=0, tmedge=1)}[path]
    script = [("step", DT, 0 if path == "schedule0" else 1)] * 3
    exact = 1 if path == "exact" else 0
    on, gens = _run(st, dict(opts, stepkeep=stepkeep), script, exact)
    assert gens == [0, 0, 0]
    off, _ = _run(st, dict(opts, stepkeep=0), script, exact)
    _same(on, off, path)


def test_stepkeep_three_subdomains(x1_2562):
    """three loopback subdomains: generation 0 in every step, the fields of one context, the same exchange
    counts with stepkeep 0, 1 and 2"""
    st = _state(x1_2562, 56, "random")

    def step(stepkeep, gens):
        def fn(c):
            c.set_option("hfuse", 0)
            c.set_option("stepkeep", stepkeep)
            for n in range(3):
                T.atm_srk3(c, DT, 1)
                assert c.get_option("stepkeep_gen") == gens[n]
        return fn
    runs = [run_decomposed(st, 3, step(k, (0, 0, 0)), 0) for k in (0, 1, 2)]
    assert all(s[0] > 0 for s in runs[0][1])  # the halo was exercised
    assert runs[0][1] == runs[1][1] == runs[2][1]
    one = run_single(st, step(2, (1, 2, 2)), 0)
    for got, _ in runs:
        bad = compare_states(got, one, rtol=0.0)
        assert not bad, bad[:6]


def test_stepkeep_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("stepkeep") == 1 and ctx.get_option("stepkeep_gen") == 0  # the defaults
        for bad in (3, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("stepkeep", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("stepkeep") == 1
        for v in (0, 2, 1):
            ctx.set_option("stepkeep", v)
            assert ctx.get_option("stepkeep") == v
        with pytest.raises(lib.MpasError):
            ctx.set_option("stepkeep_gen", 1)  # (read-only)
