"""Option `dynkeep`: a kept step's dyn_tend reuses what the step before stored (DESIGN §4n;
tests/test_dynkeep_identity.py is the CPU premise).

Where `a0keep` is active and `stepkeep` is 1, the kept steps launch guarded instances of stage 0's edge kernel, its
C and the three stages' E.  Each loads a device flag first.  The first kept step after a full one finds it 0, runs
the kernels as without the option and also leaves tend_u_euler (before the deferred del4) and each stage's w in
scratch columns, then sets the flag; the later kept steps find it 1, copy those columns back and form nothing else.
A full step clears the flag.  The launches of all kept steps are the same -- one captured graph, the timing keys of
`dynkeep` 0 -- and every field keeps its bits against `dynkeep` 0 and against `stepkeep` 0.  The parity also runs
on the states with u and v scaled by 1e-6, where what stage 0 stores in step 1 differs from step 2's nearly
everywhere.  The small mesh runs with hfuse = 0 (its default, the combined launches, is an inactive path).
"""
import os
import sys

import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_a0keep_identity import WIND
from test_gpu_a0keep import _any_state, _twin5
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state
from test_gpu_stepkeep import _run, _same, _timing, _upload

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 720.0
DYN = "atm_compute_dyn_tend_work"
TAGS = ["[rk0+copy+d4o+ntu]", "[rk>0+d4i+v]", "[rk>0+ntu]"]  # (the rows tests/test_gpu_bench.py pins)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("variant", ["random", "physical", "random-wind", "physical-wind"])
@pytest.mark.parametrize("L", [5, 56])
def test_dynkeep_bit_identical(x1_2562, L, variant, graph):
    """dynkeep 1 against 0, and both against stepkeep 0: every field after each of five consecutive steps (step 2
    fills the columns, steps 3 to 5 take the short paths)"""
    st = _any_state(x1_2562, L, variant)
    keep_check = 1 if (graph == 0 and L == 56 and variant == "random-wind") else 0  # (eager launches, once)
    on, gens = _run(st, dict(hfuse=0, graph=graph, dynkeep=1, keep_check=keep_check), ["step"] * 5)
    assert gens == [1, 2, 2, 2, 2]
    off, gens0 = _run(st, dict(hfuse=0, graph=graph, dynkeep=0), ["step"] * 5)
    assert gens0 == gens
    twin = _twin5(x1_2562, L, variant, graph)
    _same(on, off, "dynkeep 1 / 0")
    _same(on, twin, "dynkeep 1 / stepkeep 0")
    _same(off, twin, "dynkeep 0 / stepkeep 0")


@pytest.mark.parametrize("graph", [0, 1])
def test_dynkeep_flag(x1_2562, graph):
    """the device flag: 0 after a full step, 1 after every kept one; an outside call leads to a full step, which
    clears it; with dynkeep 0 no step writes it"""
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.set_option("graph", graph)
        ctx.upload(st)
        assert ctx.get_option("dynkeep_fresh") == 0
        seen = []
        for _ in range(3):
            T.atm_srk3(ctx, DT, 1)
            seen.append(ctx.get_option("dynkeep_fresh"))
        assert seen == [0, 1, 1]
        assert ctx.get_option("stepkeep_gen") == 2  # (reading the flag is no outside call)
        ctx.upload(st, names=["u"])
        assert ctx.get_option("dynkeep_fresh") == 1  # (stale by the host's count; the full step comes first)
        T.atm_srk3(ctx, DT, 1)
        assert ctx.get_option("dynkeep_fresh") == 0 and ctx.get_option("stepkeep_gen") == 1
        T.atm_srk3(ctx, DT, 1)
        assert ctx.get_option("dynkeep_fresh") == 1
        ctx.set_option("dynkeep", 0)
        for _ in range(3):
            T.atm_srk3(ctx, DT, 1)
            assert ctx.get_option("dynkeep_fresh") == 1  # (nothing reads or writes it)
        with pytest.raises(lib.MpasError):
            ctx.set_option("dynkeep_fresh", 1)  # (read-only)


def _dynkeep_101(ctx, other):
    ctx.set_option("dynkeep", 0)
    ctx.set_option("dynkeep", 1)


def _dynkeep_step(ctx, other):
    ctx.set_option("dynkeep", 0)
    T.atm_srk3(ctx, DT, 1)
    ctx.set_option("dynkeep", 1)


def _other_dt(ctx, other):
    T.atm_srk3(ctx, 360.0, 1)


CHANGES = {
    **{"upload_" + n: _upload(n) for n in ("u", "w", "theta_m", "divergence", "tend_u_euler", "delsq_u", "tend_w_euler")},
    "fill": lambda ctx, other: ctx.fill_synthetic(4242),
    "dyn_tend": lambda ctx, other: T.atm_compute_dyn_tend_work(ctx, 0, DT),
    "dynkeep_101": _dynkeep_101,
    "dynkeep_step": _dynkeep_step,
    "other_dt": _other_dt,
    "timing": _timing,
}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_dynkeep_invalidation(x1_2562, change):
    """three steps, one call from outside, two steps: every field after every step equals the stepkeep 0 twin given
    the same calls"""
    L = 56
    st = _any_state(x1_2562, L, "random-wind")
    other = make_state(x1_2562, L, "random", seed=77)  # (another state: every uploaded field differs from st's)
    other["u"][...] *= 3.0 * WIND
    gen_after = []

    def act(ctx):
        CHANGES[change](ctx, other)
        gen_after.append(ctx.get_option("stepkeep_gen"))
    script = ["step"] * 3 + [act] + ["step"] * 2
    on, gens = _run(st, dict(hfuse=0, dynkeep=1), script)
    if change == "timing":  # (the eager step takes the same decisions, on the same flag: the generation goes on)
        assert gen_after == [2] and gens == [1, 2, 2, 2, 2]
    else:
        # (another dt: that step ran full and left generation 1 for its own dt; the next 720 s step starts at 0)
        assert gen_after == ([1] if change == "other_dt" else [0]) and gens == [1, 2, 2, 1, 2]
    gen_after.clear()
    off, gens0 = _run(st, dict(hfuse=0, stepkeep=0), script)
    assert gens0 == [0] * 5
    _same(on, off, change)
    if change in ("upload_u", "upload_theta_m", "fill"):  # ... and the new values reached the step
        assert compare_states(_twin5(x1_2562, L, "random-wind", 1)[4], off[4], rtol=0.0)


def _timed_steps(st, dynkeep, n=3):
    reps = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.set_option("dynkeep", dynkeep)
        ctx.upload(st)
        ctx.timing(True)
        for _ in range(n):
            ctx.timing_reset()
            T.atm_srk3(ctx, DT, 1)
            ctx.sync()
            reps.append(ctx.timing_report())
    return reps


def test_dynkeep_timing_rows(x1_2562):
    """no timing key of its own: the kept steps' key sets are equal and are those of dynkeep 0; bench.py's table
    reports the three dyn_tend launches with the pinned tags"""
    sys.path.insert(0, REPO)
    import bench
    st = _state(x1_2562, 5, "random")
    on, off = _timed_steps(st, 1), _timed_steps(st, 0)
    live = [{k for k, (calls, _) in r.items() if calls} for r in on]
    live0 = [{k for k, (calls, _) in r.items() if calls} for r in off]
    assert live[1] == live[2]
    assert live == live0
    for r, names in zip(on, live):
        t = bench.task_table({k: r[k] for k in names}, st.dims(), 1, physics=0, ddx=True)
        assert t[DYN]["launches_per_step"] == 3
        assert sum(calls for k, (calls, _) in r.items() if k.startswith(DYN)) == 3
        tags = sorted(k[len(DYN):].replace("-A]", "]") for k in names if k.startswith(DYN))
        assert tags == TAGS, tags


def test_dynkeep_graph_counts(x1_2562):
    """the kept steps share one capture whether they fill the columns or read them: two per (dt, schedule)"""
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.upload(st)
        assert ctx.get_option("dynkeep") == 1  # the default
        n = 0
        for dt, steps, caps in ((720.0, 6, 2), (360.0, 4, 4), (720.0, 4, 4)):
            for _ in range(steps):
                T.atm_srk3(ctx, dt, 1)
            n += steps
            ctx.sync()
            assert ctx.get_option("graph_captures") == caps, (dt, steps)
            assert ctx.get_option("graph_launches") == n


@pytest.mark.parametrize("variant", ["random-wind", "physical-wind"])
def test_dynkeep_stepkeep2(x1_2562, variant):
    """stepkeep 2 keeps its own host-side launches (and X_w0) with the option on"""
    L = 56
    on, gens = _run(_any_state(x1_2562, L, variant), dict(hfuse=0, stepkeep=2, dynkeep=1), ["step"] * 5)
    assert gens == [1, 2, 2, 2, 2]
    _same(on, _twin5(x1_2562, L, variant, 1), "stepkeep 2")


@pytest.mark.parametrize("path", ["exact", "physics1", "hfuse"])
def test_dynkeep_inactive_paths(x1_2562, path):
    """where stepkeep is not active the option changes nothing: generation 0, the flag untouched, the fields of
    dynkeep 0"""
    st = mpas_state(x1_2562, 5, "mpas0") if path == "physics1" else _state(x1_2562, 5, "random")
    opts = {"exact": dict(hfuse=0), "physics1": dict(hfuse=0, physics=1), "hfuse": dict(hfuse=1)}[path]
    exact = 1 if path == "exact" else 0
    fresh = []
    script = ["step"] * 3 + [lambda ctx: fresh.append(ctx.get_option("dynkeep_fresh"))]
    on, gens = _run(st, dict(opts, dynkeep=1), script, exact)
    assert gens == [0, 0, 0] and fresh == [0]
    off, _ = _run(st, dict(opts, dynkeep=0), script, exact)
    _same(on, off, path)


def test_dynkeep_three_subdomains(x1_2562):
    """three loopback subdomains: generation 0 in every step, the fields of one context, the same exchange counts
    with dynkeep 0 and 1"""
    st = _any_state(x1_2562, 56, "random-wind")

    def step(dynkeep, gens):
        def fn(c):
            c.set_option("hfuse", 0)
            c.set_option("dynkeep", dynkeep)
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


def test_dynkeep_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("dynkeep") == 1  # the default
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("dynkeep", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("dynkeep") == 1
        for v in (0, 1):
            ctx.set_option("dynkeep", v)
            assert ctx.get_option("dynkeep") == v
