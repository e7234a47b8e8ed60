"""Option `a0keep`: the kept steps' missing stage-0 A launch and edge finish (DESIGN §4m;
tests/test_a0keep_identity.py is the CPU premise).

Where `stepkeep` is active, a step at generation >= 1 runs stage 0's dyn_tend without kernel A and without the
orphan-edge copy: tend_rho, dpdz, the w scratch, ru_save and u_2 hold the bytes the step before stored, and B stays
the instance that loads neither u nor ru.  kdiff is the exception -- it reads v, which stage 2 of the first step
replaces -- so the full step ends with one launch that forms the next step's kdiff into a scratch column, and the
kept setup launch copies it into the field.  The finish of a kept step runs its cell part alone.  Every field
keeps its bits against a0keep 0 and against stepkeep 0.  The stock states have kdiff at its cap everywhere, so the
parity also runs on states with u and v scaled by 1e-6, where kdiff after step 1 differs from step 2 nearly
everywhere.  The small mesh runs with hfuse = 0 (its default, the combined launches, is an inactive path).
"""
import os
import sys

import numpy as np
import pytest

from helpers import compare_states
from mpasdyn import lib
from mpasdyn import tasks as T
from test_a0keep_identity import scaled_state
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state
from test_gpu_stepkeep import _off5, _run, _same, _toggle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 720.0
DYN0 = "atm_compute_dyn_tend_work[rk0+copy+d4o+ntu]"
DYN0_NOA = "atm_compute_dyn_tend_work[rk0+copy+d4o+ntu-A]"
KDIFF = "a0keep_kdiff"
_SC, _SC_OFF = {}, {}


def _any_state(mesh, L, variant):
    """the two stock variants, and `<variant>-wind`: u and v scaled so that kdiff leaves its cap"""
    if not variant.endswith("-wind"):
        return _state(mesh, L, variant)
    key = (L, variant)
    if key not in _SC:
        _SC[key] = scaled_state(mesh, L, variant[:-5])
    return _SC[key]


def _twin5(mesh, L, variant, graph):
    """five steps with stepkeep 0: computed once per case, never modified"""
    if not variant.endswith("-wind"):
        return _off5(mesh, L, variant, graph)
    key = (L, variant, graph)
    if key not in _SC_OFF:
        _SC_OFF[key] = _run(_any_state(mesh, L, variant), dict(hfuse=0, graph=graph, stepkeep=0), ["step"] * 5)[0]
    return _SC_OFF[key]


def _kdiff_moved(a, b):
    """the fraction of the points of rows < nCells, levels < L at which kdiff differs"""
    n, L = a.dims()[0], a.L
    with np.errstate(invalid="ignore"):
        return float(np.mean(a["kdiff"][:n, :L] != b["kdiff"][:n, :L]))


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("variant", ["random", "physical", "random-wind", "physical-wind"])
@pytest.mark.parametrize("L", [5, 56])
def test_a0keep_bit_identical(x1_2562, L, variant, graph):
    """a0keep 1 against 0, and both against stepkeep 0: every field after each of five consecutive steps"""
    st = _any_state(x1_2562, L, variant)
    keep_check = 1 if (graph == 0 and L == 56 and variant == "random-wind") else 0  # (eager launches, once)
    on, gens = _run(st, dict(hfuse=0, graph=graph, a0keep=1, keep_check=keep_check), ["step"] * 5)
    assert gens == [1, 2, 2, 2, 2]
    off, gens0 = _run(st, dict(hfuse=0, graph=graph, a0keep=0), ["step"] * 5)
    assert gens0 == gens
    twin = _twin5(x1_2562, L, variant, graph)
    if variant.endswith("-wind"):  # (not vacuous: the kept steps need another kdiff than step 1 left)
        frac = _kdiff_moved(twin[0], twin[1])
        print("kdiff differs between steps 1 and 2 at", frac, "of the points")
        assert frac >= 0.90
    _same(on, off, "a0keep 1 / 0")
    _same(on, twin, "a0keep 1 / stepkeep 0")
    _same(off, twin, "a0keep 0 / stepkeep 0")


@pytest.mark.parametrize("variant", ["random-wind", "physical-wind"])
def test_a0keep_stepkeep2(x1_2562, variant):
    """stepkeep 2 on the scaled state: generation 1 takes the A skip, generation 2 has no stage 0"""
    L = 56
    on, gens = _run(_any_state(x1_2562, L, variant), dict(hfuse=0, stepkeep=2, a0keep=1), ["step"] * 5)
    assert gens == [1, 2, 2, 2, 2]
    _same(on, _twin5(x1_2562, L, variant, 1), "stepkeep 2")


def _upload_kept(ctx, other):
    ctx.upload(other, names=["u", "v", "ru", "rw", "rho_zz", "kdiff", "ruAvg", "ruAvg_split", "tend_rho_physics"])


def _a0keep_101(ctx, other):
    ctx.set_option("a0keep", 0)
    ctx.set_option("a0keep", 1)


CHANGES = {
    "upload": _upload_kept,
    "fill": lambda ctx, other: ctx.fill_synthetic(4242),
    "dyn_tend": lambda ctx, other: T.atm_compute_dyn_tend_work(ctx, 0, DT),
    "substep_finish": lambda ctx, other: T.atm_rk_dynamics_substep_finish(ctx, 1, 1),
    "a0keep_101": _a0keep_101,
    "a0keep_step": _toggle("a0keep", 0),
    "other_dt": lambda ctx, other: T.atm_srk3(ctx, 360.0, 1),
}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_a0keep_invalidation(x1_2562, change):
    """three steps, one call from outside, two steps: every field after every step equals the stepkeep 0 twin
    given the same calls, and the step after the call is a full one"""
    L = 56
    st = _any_state(x1_2562, L, "random-wind")
    other = scaled_state(x1_2562, L, "physical")
    other["u"][...] *= 3.0  # (another kdiff below the cap)
    other["v"][...] *= 3.0
    gen_after = []

    def act(ctx):
        CHANGES[change](ctx, other)
        gen_after.append(ctx.get_option("stepkeep_gen"))
    script = ["step"] * 3 + [act] + ["step"] * 2
    on, gens = _run(st, dict(hfuse=0, a0keep=1), script)
    # (another dt: that step ran full and left generation 1 for its own dt; the next 720 s step starts at 0)
    assert gen_after == ([1] if change == "other_dt" else [0])
    assert gens == [1, 2, 2, 1, 2]
    gen_after.clear()
    off, gens0 = _run(st, dict(hfuse=0, stepkeep=0), script)
    assert gens0 == [0] * 5
    _same(on, off, change)
    if change in ("upload", "fill"):  # ... and the new values reached the step: without the call it ends elsewhere
        assert compare_states(_twin5(x1_2562, L, "random-wind", 1)[4], off[4], rtol=0.0)


def test_a0keep_timing_rows(x1_2562):
    """step 1 has the untagged stage-0 row and the kdiff launch's; the kept steps have equal key sets, with stage
    0's dyn_tend tagged -A and without the kdiff key; bench.py's table takes every key"""
    sys.path.insert(0, REPO)
    import bench
    st = _state(x1_2562, 5, "random")
    reps = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.upload(st)
        ctx.timing(True)
        for _ in range(3):
            ctx.timing_reset()
            T.atm_srk3(ctx, DT, 1)
            ctx.sync()
            reps.append(ctx.timing_report())
    live = [{k for k, (calls, _) in r.items() if calls} for r in reps]
    assert DYN0 in live[0] and DYN0_NOA not in live[0] and KDIFF in live[0]
    assert live[1] == live[2]
    assert DYN0_NOA in live[1] and DYN0 not in live[1] and KDIFF not in live[1]
    assert not any(k.startswith("stepkeep_") or "vikeep" in k for k in live[0] | live[1])
    fin = {k for k in live[0] if k.startswith("atm_rk_dynamics_substep_finish")}  # (the finish keeps its key)
    assert len(fin) == 1 and fin <= live[1]
    for r, names in zip(reps, live):
        t = bench.task_table({k: r[k] for k in names}, st.dims(), 1, physics=0, ddx=True)
        assert t["atm_compute_dyn_tend_work"]["launches_per_step"] == 3
        assert (KDIFF in t) == (KDIFF in names)


def test_a0keep_graph_counts(x1_2562):
    """generations 1 and 2 share one capture: two per (dt, schedule), then replays"""
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.upload(st)
        n = 0
        for dt, steps, caps in ((720.0, 6, 2), (360.0, 4, 4), (720.0, 4, 4)):
            for _ in range(steps):
                T.atm_srk3(ctx, dt, 1)
            n += steps
            ctx.sync()
            assert ctx.get_option("graph_captures") == caps, (dt, steps)
            assert ctx.get_option("graph_launches") == n


@pytest.mark.parametrize("path", ["hfuse", "exact", "schedule0", "physics1", "physics2"])
def test_a0keep_inactive_paths(x1_2562, path):
    """where stepkeep is not active the option changes nothing: generation 0, the fields of a0keep 0"""
    mpas = path.startswith("physics")
    st = mpas_state(x1_2562, 5, "mpas0") if mpas else _state(x1_2562, 5, "random")
    opts = {"hfuse": dict(hfuse=1), "exact": dict(hfuse=0), "schedule0": dict(hfuse=0), "physics1": dict(hfuse=0, physics=1),
            "physics2": dict(hfuse=0, physics=2)}[path]
    script = [("step", DT, 0 if path == "schedule0" else 1)] * 3
    exact = 1 if path == "exact" else 0
    on, gens = _run(st, dict(opts, a0keep=1), script, exact)
    assert gens == [0, 0, 0]
    off, _ = _run(st, dict(opts, a0keep=0), script, exact)
    _same(on, off, path)


def test_a0keep_three_subdomains(x1_2562):
    """three loopback subdomains: generation 0 in every step, the fields of one context, the same exchange
    counts with a0keep 0 and 1"""
    st = _any_state(x1_2562, 56, "random-wind")

    def step(a0keep, gens):
        def fn(c):
            c.set_option("hfuse", 0)
            c.set_option("a0keep", a0keep)
            for n in range(3):
                T.atm_srk3(c, DT, 1)
                assert c.get_option("stepkeep_gen") == gens[n]
        return fn
    runs = [run_decomposed(st, 3, step(k, (0, 0, 0)), 0) for k in (0, 1)]
    assert all(s[0] > 0 for s in runs[0][1])  # the halo was exercised
    assert runs[0][1] == runs[1][1]
    one = run_single(st, step(1, (1, 2, 2)), 0)
    for got, _ in runs:
        bad = compare_states(got, one, rtol=0.0)
        assert not bad, bad[:6]


def test_a0keep_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("a0keep") == 1  # the default
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("a0keep", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("a0keep") == 1
        for v in (0, 1):
            ctx.set_option("a0keep", v)
            assert ctx.get_option("a0keep") == v
