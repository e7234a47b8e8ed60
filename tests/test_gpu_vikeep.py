"""Option `vikeep` and the kept steps' missing stage-2 A launch (tests/test_vikeep_identity.py is
the CPU premise).

Where `stepkeep` is active, stage 0's vert_imp coefficient set lives in scratch columns, so the fields keep
stage 1's; from the second consecutive step on both vert_imp launches form alpha_tri and gamma_tri alone from
the stored a, b, c, and stage 2's dyn_tend runs without its kernel A (h_divergence is a function of ru and the
mesh).  Every field keeps its bits against vikeep 0 and against stepkeep 0, the step with every launch; every
call from outside that could change an input sends the generation back to 0, and the full step that follows
rewrites every kept column before it is read.  The small mesh runs with hfuse = 0 (its default, the combined
launches, is one of the inactive paths).
"""
import os
import sys

import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state
from test_gpu_stepkeep import _off5, _run, _same, _toggle, _upload

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 720.0
NOA = "atm_compute_dyn_tend_work[rk>0+d4i+v-A]"


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 56])
def test_vikeep_bit_identical(x1_2562, L, variant, graph):
    """vikeep 1 against 0, and both against stepkeep 0: every field after each of five consecutive steps"""
    st = _state(x1_2562, L, variant)
    keep_check = 1 if (graph == 0 and L == 56 and variant == "random") else 0  # (eager launches, once)
    on, gens = _run(st, dict(hfuse=0, graph=graph, vikeep=1, keep_check=keep_check), ["step"] * 5)
    assert gens[:3] == [1, 2, 2] and gens == [1, 2, 2, 2, 2]
    off, gens0 = _run(st, dict(hfuse=0, graph=graph, vikeep=0), ["step"] * 5)
    assert gens0 == gens
    _same(on, off, "vikeep 1 / 0")
    _same(on, _off5(x1_2562, L, variant, graph), "vikeep 1 / stepkeep 0")


def _other_dt(ctx, other):
    T.atm_srk3(ctx, 360.0, 1)


CHANGES = {
    **{"upload_" + n: _upload(n) for n in ("zz", "theta_m", "rtheta_p", "exner", "a_tri", "cofwt", "gamma_tri", "ru",
                                           "h_divergence")},
    "fill": lambda ctx, other: ctx.fill_synthetic(4242),
    "vert_imp_coefs": lambda ctx, other: T.atm_compute_vert_imp_coefs(ctx, 77.0),
    "integration_setup": lambda ctx, other: T.atm_rk_integration_setup(ctx),
    "vikeep": _toggle("vikeep", 0),
    "accoef": _toggle("accoef", 0),
    "other_dt": _other_dt,
}
_TWIN = {}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_vikeep_invalidation(x1_2562, change):
    """three steps, one call from outside, two steps: every field after every step equals the stepkeep 0 twin
    given the same calls, and the step after the call is a full one"""
    L = 56
    st = _state(x1_2562, L, "random")
    other = make_state(x1_2562, L, "random", seed=77)
    gen_after = []

    def act(ctx):
        CHANGES[change](ctx, other)
        gen_after.append(ctx.get_option("stepkeep_gen"))
    script = ["step"] * 3 + [act] + ["step"] * 2
    on, gens = _run(st, dict(hfuse=0, vikeep=1), script)
    # (another dt: that step ran full and left generation 1 for its own dt; the next 720 s step starts at 0)
    assert gen_after == ([1] if change == "other_dt" else [0])
    assert gens == [1, 2, 2, 1, 2]
    gen_after.clear()
    off, gens0 = _run(st, dict(hfuse=0, stepkeep=0), script)
    assert gens0 == [0] * 5
    _same(on, off, change)
    if change in ("upload_zz", "upload_theta_m", "upload_rtheta_p", "upload_exner", "upload_ru", "fill"):
        # ... and the new values reached the step: without the call it ends elsewhere
        if "plain" not in _TWIN:
            _TWIN["plain"] = _run(st, dict(hfuse=0, stepkeep=0), ["step"] * 5)[0]
        assert compare_states(_TWIN["plain"][4], off[4], rtol=0.0)


def test_vikeep_timing_rows(x1_2562):
    """under per-task timing the kept steps have equal key sets, with stage 2's dyn_tend tagged -A and no key of
    the option's own; bench.py's table takes every key"""
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
    assert live[1] == live[2]
    assert NOA in live[1] and NOA not in live[0] and NOA.replace("-A]", "]") in live[0]
    assert not any(k.startswith("stepkeep_") or "vikeep" in k for k in live[0] | live[1])
    for name in ("atm_rk_integration_setup[cells+moist+vert_imp-bc]", "atm_compute_vert_imp_coefs"):
        assert all(name in s for s in live)
    for r, names in zip(reps, live):
        t = bench.task_table({k: r[k] for k in names}, st.dims(), 1, physics=0, ddx=True)
        assert t["atm_compute_dyn_tend_work"]["launches_per_step"] == 3


def test_vikeep_graph_counts(x1_2562):
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
def test_vikeep_inactive_paths(x1_2562, path):
    """where stepkeep is not active the option changes nothing: generation 0, the fields of vikeep 0"""
    mpas = path.startswith("physics")
    st = mpas_state(x1_2562, 5, "mpas0") if mpas else _state(x1_2562, 5, "random")
    opts = {"hfuse": dict(hfuse=1), "exact": dict(hfuse=0), "schedule0": dict(hfuse=0), "physics1": dict(hfuse=0, physics=1),
            "physics2": dict(hfuse=0, physics=2)}[path]
    script = [("step", DT, 0 if path == "schedule0" else 1)] * 3
    exact = 1 if path == "exact" else 0
    on, gens = _run(st, dict(opts, vikeep=1), script, exact)
    assert gens == [0, 0, 0]
    off, _ = _run(st, dict(opts, vikeep=0), script, exact)
    _same(on, off, path)


def test_vikeep_three_subdomains(x1_2562):
    """three loopback subdomains: generation 0 in every step, the fields of one context, the same exchange
    counts with vikeep 0 and 1"""
    st = _state(x1_2562, 56, "random")

    def step(vikeep, gens):
        def fn(c):
            c.set_option("hfuse", 0)
            c.set_option("vikeep", vikeep)
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


def test_vikeep_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("vikeep") == 1  # the default
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("vikeep", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("vikeep") == 1
        for v in (0, 1):
            ctx.set_option("vikeep", v)
            assert ctx.get_option("vikeep") == v
