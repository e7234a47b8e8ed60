"""Option `tukeep`: in a fresh kept step stage 2's edge kernel forms tend_u's top level only (DESIGN §4p;
tests/test_tukeep_identity.py is the CPU premise).

Where `dynkeep` is active, the kept steps launch guarded instances of stage 0's and stage 2's edge kernels and, right
behind the latter, `k_dyn_B_top`.  With the device flag 0 (the first kept step after a full one) the two guarded
kernels run as with `dynkeep` alone and `k_dyn_B_top` returns.  With the flag 1 stage 0's returns without copying
tend_u_euler back (it holds its final value), stage 2's returns, and `k_dyn_B_top` forms tend_u at level L - 1 from
the stored tend_u_euler: every other level, tend_u_euler and v hold the step-before's bits.  The launches of all kept
steps are the same -- one captured graph, the timing keys of `tukeep` 0 -- and every field keeps its bits against
`tukeep` 0 and against `stepkeep` 0.  The meshes run with hfuse = 0 (the small grids' default, the combined launches,
is an inactive path).
"""
import os
import sys

import numpy as np
import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import mesh as M
from mpasdyn import tasks as T
from test_a0keep_identity import WIND
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_stepkeep import _run, _same, _timing, _upload

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 720.0
DYN = "atm_compute_dyn_tend_work"
TAGS = ["[rk0+copy+d4o+ntu]", "[rk>0+d4i+v]", "[rk>0+ntu]"]  # (the rows tests/test_gpu_bench.py pins)
# x1.2562 at LP 8 and 64; the Voronoi mesh with 4- to 8-sided cells (nEdgesOnEdge up to 14 > QF, odd entity counts)
# at LP 8 and at L = 63, where level L sits in the column's last lane
CASES = [("x1.2562", 5), ("x1.2562", 56), ("irregular", 5), ("irregular", 63)]
CASE_IDS = [f"{m}-L{L}" for m, L in CASES]

_MESH, _ST, _TWIN = {}, {}, {}


def _mesh(name, x1_2562):
    if name == "x1.2562":
        return x1_2562
    if name not in _MESH:
        _MESH[name] = M.irregular()
    return _MESH[name]


def _state(x1_2562, name, L, variant):
    """`random`, and `random-wind`: u and v scaled by 1e-6 (built once per case, never modified)"""
    key = (name, L, variant)
    if key not in _ST:
        st = make_state(_mesh(name, x1_2562), L, "random")
        if variant == "random-wind":
            st["u"][...] *= WIND
            st["v"][...] *= WIND
        _ST[key] = st
    return _ST[key]


def _twin5(x1_2562, name, L, variant, graph):
    """five steps with stepkeep 0: computed once per case, never modified"""
    key = (name, L, variant, graph)
    if key not in _TWIN:
        _TWIN[key] = _run(_state(x1_2562, name, L, variant), dict(hfuse=0, graph=graph, stepkeep=0), ["step"] * 5)[0]
    return _TWIN[key]


def _probe(log):
    def fn(ctx):
        log.append((ctx.get_option("tukeep_active"), ctx.get_option("dynkeep_fresh"), ctx.get_option("stepkeep_gen")))
    return fn


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("variant", ["random", "random-wind"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tukeep_bit_identical(x1_2562, case, variant, graph):
    """tukeep 1 against 0, and both against stepkeep 0: every field after each of five consecutive steps (step 2 is
    the stale pass, steps 3 to 5 take the short path); the option's state, the flag and the generation after each;
    and the short path ran on evolving data"""
    name, L = case
    st = _state(x1_2562, name, L, variant)
    log, log0 = [], []
    script = [x for _ in range(5) for x in ("step", _probe(log))]
    keep_check = 1 if (graph == 0 and variant == "random") else 0  # (eager launches)
    on, gens = _run(st, dict(hfuse=0, graph=graph, tukeep=1, keep_check=keep_check), script)
    assert gens == [1, 2, 2, 2, 2]
    assert log == [(1, 0, 1), (1, 1, 2), (1, 1, 2), (1, 1, 2), (1, 1, 2)]
    script0 = [x for _ in range(5) for x in ("step", _probe(log0))]
    off, gens0 = _run(st, dict(hfuse=0, graph=graph, tukeep=0), script0)
    assert gens0 == gens
    assert log0 == [(0, f, g) for _, f, g in log]
    twin = _twin5(x1_2562, name, L, variant, graph)
    _same(on, off, "tukeep 1 / 0")
    _same(on, twin, "tukeep 1 / stepkeep 0")
    _same(off, twin, "tukeep 0 / stepkeep 0")
    # the ends of steps 3 and 4, both fresh passes: tend_u moved at level L - 1 and nowhere else
    a, b = on[2]["tend_u"], on[3]["tend_u"]
    nE = st.dims()[1]
    keep = np.ones(a.shape[1], dtype=bool)
    keep[L - 1] = False
    assert a[:, keep].tobytes() == b[:, keep].tobytes()
    moved = int(np.sum(a[:nE, L - 1].view(np.uint64) != b[:nE, L - 1].view(np.uint64)))
    print(f"{name} L {L} {variant}: tend_u(L - 1) differs at {moved} of {nE} edges between steps 3 and 4")
    if variant == "random":
        assert moved > nE // 2


def _tukeep_101(ctx, other):
    ctx.set_option("tukeep", 0)
    ctx.set_option("tukeep", 1)


def _tukeep_step(ctx, other):
    ctx.set_option("tukeep", 0)
    T.atm_srk3(ctx, DT, 1)
    ctx.set_option("tukeep", 1)


def _dynkeep_off(ctx, other):
    ctx.set_option("dynkeep", 0)
    assert ctx.get_option("tukeep") == 1 and ctx.get_option("tukeep_active") == 0


def _other_dt(ctx, other):
    T.atm_srk3(ctx, 360.0, 1)


CHANGES = {
    **{"upload_" + n: _upload(n) for n in ("tend_u", "tend_u_euler", "v", "w", "u")},
    "fill": lambda ctx, other: ctx.fill_synthetic(4242),
    "dyn_tend": lambda ctx, other: T.atm_compute_dyn_tend_work(ctx, 0, DT),
    "tukeep_101": _tukeep_101,
    "tukeep_step": _tukeep_step,
    "dynkeep_off": _dynkeep_off,
    "other_dt": _other_dt,
    "timing": _timing,
}


@pytest.mark.parametrize("change", sorted(CHANGES))
def test_tukeep_invalidation(x1_2562, change):
    """three steps, one call from outside, two steps: every field after every step equals the stepkeep 0 twin given
    the same calls"""
    L = 56
    st = _state(x1_2562, "x1.2562", L, "random")
    other = make_state(x1_2562, L, "random", seed=77)  # (another state: every uploaded field differs from st's)
    gen_after = []

    def act(ctx):
        CHANGES[change](ctx, other)
        gen_after.append(ctx.get_option("stepkeep_gen"))
    script = ["step"] * 3 + [act] + ["step"] * 2
    on, gens = _run(st, dict(hfuse=0, tukeep=1), script)
    if change == "timing":  # (the eager step takes the same decisions, on the same flag: the generation goes on)
        assert gen_after == [2] and gens == [1, 2, 2, 2, 2]
    else:
        # (another dt: that step ran full and left generation 1 for its own dt; the next 720 s step starts at 0)
        assert gen_after == ([1] if change == "other_dt" else [0]) and gens == [1, 2, 2, 1, 2]
    gen_after.clear()

    def act0(ctx):  # (the twin's options are its own: the toggles are no-ops on the fields there too)
        CHANGES[change](ctx, other)
    off, gens0 = _run(st, dict(hfuse=0, stepkeep=0), ["step"] * 3 + [act0] + ["step"] * 2)
    assert gens0 == [0] * 5
    _same(on, off, change)
    if change in ("upload_u", "upload_w", "fill"):  # ... and the new values reached the step
        assert compare_states(_twin5(x1_2562, "x1.2562", L, "random", 1)[4], off[4], rtol=0.0)


@pytest.mark.parametrize("timed", [(1,), (2,), (1, 3), (2, 4)], ids=lambda t: "timed" + "".join(map(str, t)))
def test_tukeep_timed_steps_interleaved(x1_2562, timed):
    """a step with per-task timing on launches `dynkeep`'s instances (its dyn_tend rows are set against the
    reference task's B_alg), whichever pass it is -- the stale one (step 2: index 1) or a fresh one -- and the
    untimed steps around it take the short path on what it left: five steps equal to the twin's, the generation
    going on, `tukeep_active` 0 while timing is on"""
    L = 56
    st = _state(x1_2562, "x1.2562", L, "random")
    active = []
    script = []
    for n in range(5):
        if n in timed:
            script.append(lambda ctx: (ctx.timing(True), active.append(ctx.get_option("tukeep_active"))))
        script.append("step")
        if n in timed:
            script.append(lambda ctx: (ctx.timing(False), active.append(ctx.get_option("tukeep_active"))))
    on, gens = _run(st, dict(hfuse=0, tukeep=1), script)
    assert gens == [1, 2, 2, 2, 2]
    assert active == [0, 1] * len(timed)
    _same(on, _twin5(x1_2562, "x1.2562", L, "random", 1), f"timed steps {timed}")


def _timed_steps(st, tukeep, n=3):
    reps = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.set_option("tukeep", tukeep)
        ctx.upload(st)
        ctx.timing(True)
        for _ in range(n):
            ctx.timing_reset()
            T.atm_srk3(ctx, DT, 1)
            ctx.sync()
            reps.append(ctx.timing_report())
    return reps


def test_tukeep_timing_rows(x1_2562):
    """no timing key of its own: the kept steps' key sets are equal and are those of tukeep 0; bench.py's table
    reports the three dyn_tend launches with the pinned tags"""
    sys.path.insert(0, REPO)
    import bench
    st = _state(x1_2562, "x1.2562", 5, "random")
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


def test_tukeep_graph_counts(x1_2562):
    """the kept steps share one capture whether they take the long or the short path: two per (dt, schedule)"""
    st = _state(x1_2562, "x1.2562", 5, "random")
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("hfuse", 0)
        ctx.upload(st)
        assert ctx.get_option("tukeep") == 1 and ctx.get_option("tukeep_active") == 1  # the default
        n = 0
        for dt, steps, caps in ((720.0, 6, 2), (360.0, 4, 4), (720.0, 4, 4)):
            for _ in range(steps):
                T.atm_srk3(ctx, dt, 1)
            n += steps
            ctx.sync()
            assert ctx.get_option("graph_captures") == caps, (dt, steps)
            assert ctx.get_option("graph_launches") == n


@pytest.mark.parametrize("path", ["exact", "physics1", "hfuse", "stepkeep2"])
def test_tukeep_inactive_paths(x1_2562, path):
    """where dynkeep is not active the option changes nothing: tukeep_active 0, the fields of tukeep 0"""
    st = mpas_state(x1_2562, 5, "mpas0") if path == "physics1" else _state(x1_2562, "x1.2562", 5, "random")
    opts = {"exact": dict(hfuse=0), "physics1": dict(hfuse=0, physics=1), "hfuse": dict(hfuse=1),
            "stepkeep2": dict(hfuse=0, stepkeep=2)}[path]
    exact = 1 if path == "exact" else 0
    log, log0 = [], []
    on, gens = _run(st, dict(opts, tukeep=1), ["step"] * 3 + [_probe(log)], exact)
    assert gens == ([1, 2, 2] if path == "stepkeep2" else [0, 0, 0])
    assert log[0][0] == 0 and log[0][1] == 0  # (inactive; nothing wrote the flag)
    off, _ = _run(st, dict(opts, tukeep=0), ["step"] * 3 + [_probe(log0)], exact)
    assert log0 == log
    _same(on, off, path)


def test_tukeep_three_subdomains(x1_2562):
    """three loopback subdomains: generation 0 in every step, the fields of one context, the same exchange counts
    with tukeep 0 and 1"""
    st = _state(x1_2562, "x1.2562", 56, "random-wind")

    def step(tukeep, gens):
        def fn(c):
            c.set_option("hfuse", 0)
            c.set_option("tukeep", tukeep)
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


def test_tukeep_option_values(x1_2562):
    st = _state(x1_2562, "x1.2562", 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("tukeep") == 1  # the default
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("tukeep", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("tukeep") == 1
        for v in (0, 1):
            ctx.set_option("tukeep", v)
            assert ctx.get_option("tukeep") == v
        with pytest.raises(lib.MpasError):
            ctx.set_option("tukeep_active", 1)  # (read-only)
