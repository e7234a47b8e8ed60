"""GPU vs oracle parity on mesh.irregular(): 647 cells with 4 to 8 edges (113 with 7, 5 with
8), 499 of 1935 edges with more than QF = 10 edgesOnEdge entries (up to 13), 1290 vertices --
the lists past the kernels' unconditional NF = 6 / QF = 10 slots, which no x1 mesh has, and
entity counts that are no multiple of any block's column count (the last block of every
undecomposed cell, edge and vertex launch is partly filled).  tests/test_irregular_mesh.py
validates the mesh and the oracle on it, and asserts the coverage this module relies on.

Levels: L = 5, 26, 63 (LP 8, 32, 64): eight, two, one column per wavefront; at LP 8 the columns
sharing a wavefront have different list lengths (tail loops of different trip counts beside
lvl_dn / lvl_up shuffles); LP 64 takes gather2 / put2 and the LP-64-only options.  Variants:
"random", "ref" (raw 1-based ids: zero slot, non-SELF gathers, orphan edge) and "mpas0"
(0-based ids: SELF gathers; selfc asserted).  The states are this module's own (the caches of
the x1.2562 modules are keyed without the mesh); their task lists, runners and tolerances are
imported unchanged.

Tail loops reached, per kernel file (`for (i = NF; i < ne; ...)`, `for (j = QF; j < neoe; ...)`):
* k_dyn.hip -- dyn_A_body's kdiff, h_divergence, ru_l and w0 tails (dyn_tend rk0 / rk1 tasks,
  every srk3 case) and its CPA copy tail with `own >> i`, i >= NF (test_irr_copies_by_A, which
  asserts from the host that an edge is owned through such a slot); B's edgesOnEdge tails
  (:554, :566: dyn_tend tasks; 499 edges); E's lvl_dn tail (:902) and the tails of E's flux
  sums, reference and MPAS forms (:1199-:1383: the dyn_tend tasks of both TASKS lists, exact
  and fast).  etile's tiled E is not built here (tiles_build refuses a cell with more than NF
  edges: test_irr_etile_inactive), so the untiled E runs for the mesh's sake.
* k_cols.h -- the column forms of the same sums used by the fused launches (:453, :520, :587):
  test_irr_fusion_options (hfuse / fusesetup / fusesml) and the default small-mesh hfuse order
  of every srk3 case.
* k_acoustic.hip -- the fused set_smlstep's tail (SML 1: every exact srk3 case) and the flux tail
  (the divergence of ru_p: acoustic tasks, every srk3 case, physics 0, 1, 2), which under option
  fusedamp (MODE 2: the default of every reference srk3 case) also applies the previous substep's
  damping to the slot's edge and stores it where the cell owns the edge.
* k_misc.hip -- :319 (set_smlstep / setup family) and k_prepare's cell records, which hold
  min(nEdgesOnCell, NF) edges (every upload).
* k_diag.hip -- :489 (solve_diagnostics' divergence / ke) and recover_w_col's
  `for (i = NF; i < 10; i++)` block (:228: test_irr_recover, test_irr_mpas_recover).
* k_transport.hip -- :525, :635, :678, :788 (bounds, scale and update kernels of the monotonic
  task and the unlimited stage: test_irr_transport_*); the tiled transport is not built
  (trtile_active == 0 asserted); the edge groups of tredge are built at LP 64
  (test_irr_transport_edge_groups; tredge_irregular is printed).
Not reached by any case: tre_build's irregular groups (tredge_irregular reads 0 on this mesh with
either id convention: no group's union of cells outgrows the LDS columns; x1.2562's random-id case
in test_gpu_transport.py reaches them), advCellsForEdge lists longer than AF = 9 (no mesh task
produces them),
the RCCL / socket halo transports, and 9- or 10-sided cells (the generator refuses them:
build_state's restatement of the reference's list construction overflows there).

Parameters dropped: L = 26 in the fusion-option, decomposition, etile and edge-group cases --
LP 32 instantiates the same templates as LP 8 with another LP, and those cases compare
launch orders, not list lengths; the per-task and whole-step cases keep all three levels.

Fast-path cases print `FASTERR <case> <field> <max|got - ref| / max|ref|>` before asserting."""
import numpy as np
import pytest

import oracle as O
import transport_ref as R
from helpers import SCRATCH, ZERO_SLOT_WRITTEN, compare_states, make_state, transport_state
from mpasdyn import lib
from mpasdyn import mesh as M
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import RTOL_EXTREME
from test_gpu_mpas_dynamics import TASKS as DYN_TASKS
from test_gpu_mpas_dynamics import run_gpu as run_gpu_dyn
from test_gpu_parity import (MESH_TASKS, POW_FIELDS, RTOL_FAST, RTOL_POW, RTOL_STEP, TASKS, _summary_gpu,
                             _two_steps_gpu, run_gpu, run_gpu_mpas, run_oracle)
from test_gpu_transport import gpu as gpu_tr
from test_gpu_transport_rk3 import check_task as check_transport_task

pytestmark = pytest.mark.gpu

NF = 6
LEVELS = [5, 26, 63]
L_IDS = ["L5", "L26", "L63"]
ENDS = [5, 63]
END_IDS = ["L5", "L63"]
DT = 600.0

_MESH = {}
_ST = {}


def irregular():
    if "m" not in _MESH:
        _MESH["m"] = M.irregular()
        _MESH["m0"] = M.zero_based(_MESH["m"])
    return _MESH["m"]


def state(L, variant, solver=False):
    """this module's states (built once, never modified): "random" / "ref" on the raw ids,
    "mpas0" the random state on 0-based ids; solver: with a factored MPAS vertical system"""
    key = (L, variant, solver)
    if key not in _ST:
        m = irregular()
        st = make_state(_MESH["m0"], L, "random") if variant == "mpas0" else make_state(m, L, variant)
        if solver:
            O.Oracle(st).mpas_vert_imp_coefs(240.0)
        _ST[key] = st
    return _ST[key]


def report_fast(case, got, ref, fields=None):
    for name in sorted(fields or ref.arrays):
        a, b = got.arrays[name], ref.arrays[name]
        if b.dtype != np.float64 or name in SCRATCH:
            continue
        if name in ZERO_SLOT_WRITTEN:  # (compared on the entities only, helpers.py)
            a, b = a[:-1], b[:-1]
        fin = np.isfinite(b) & np.isfinite(a)
        scale = float(np.max(np.abs(b[fin]))) if fin.any() else 0.0
        err = float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0
        if err > 0.0:
            print(f"FASTERR {case} {name} {err / max(scale, 1e-300):.3e}")


# ------------------------------------------------------------------ the mesh as the device sees it
@pytest.mark.parametrize("variant,expect", [("random", 0), ("ref", 0), ("mpas0", 1)])
def test_irr_self_gathers_detected(variant, expect):
    st = state(5, variant)
    with lib.Context(*st.dims()) as ctx:
        ctx.upload(st)
        assert ctx.get_option("selfc") == expect
        assert ctx.get_option("orphan_edges") == (0 if variant == "mpas0" else 1)


# ------------------------------------------------------------------ 1. reference tasks
@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("task", TASKS, ids=[t[0] for t in TASKS])
def test_irr_task(L, variant, task):
    name, ofn, gfn, tol_fields = task
    st = state(L, variant)
    ref = run_oracle(st, ofn)
    got = run_gpu(st, gfn, exact=1)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, f"{name}: GPU differs from oracle: {bad[:6]}"
    got.check_zero_slots()
    if tol_fields and variant != "ref":
        got = run_gpu(st, gfn, exact=0)
        report_fast(f"{name}-{variant}-L{L}", got, ref, tol_fields)
        bad = compare_states(got, ref, rtol=RTOL_FAST, tol_fields=tol_fields)
        assert not bad, f"{name}: fast path outside {RTOL_FAST}: {bad[:6]}"


# ------------------------------------------------------------------ 2. operators beside the loop
@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("ns,rk_step", [(1, 0), (3, 2)])
def test_irr_recover(L, variant, ns, rk_step):
    """recover_w_col's slots NF..9 on cells with 7 and 8 edges"""
    st = state(L, variant)
    ref = run_oracle(st, lambda o: o.atm_recover_large_step_variables_work(ns, rk_step, 240.0))
    assert variant == "mpas0" or (st["cellsOnEdge"][:st.nEdges] == st.nCells).any()
    for exact in (1, 0):
        got = run_gpu(st, lambda c: T.atm_recover_large_step_variables_work(c, ns, rk_step, 240.0), exact=exact)
        bad = compare_states(got, ref, rtol=RTOL_POW, tol_fields=POW_FIELDS, zero_slot_excluded=ZERO_SLOT_WRITTEN)
        assert not bad, f"recover ns={ns} rk={rk_step} exact={exact}: {bad[:6]}"
        got.check_zero_slots(written=("rho_zz",))
    assert (ref["rho_zz"][st.nCells, :L] == 1.0).all()


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("on_a_sphere", [True, False])
def test_irr_reconstruct_2d(L, variant, on_a_sphere):
    st = state(L, variant)
    ref = run_oracle(st, lambda o: o.mpas_reconstruct_2d(False, on_a_sphere))
    got = run_gpu(st, lambda c: T.mpas_reconstruct_2d(c, False, on_a_sphere), exact=0)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, f"reconstruct_2d: {bad[:6]}"
    got.check_zero_slots()


@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("task", list(MESH_TASKS))
def test_irr_mesh_tasks(variant, task):
    """the device mesh tasks (k_mesh.hip) with random deriv_two; advection lists of 4 to 9 cells"""
    ofn, gfn, tf = MESH_TASKS[task]
    st = state(5, variant).copy()
    nE = st.nEdges
    st["deriv_two"][:nE] = np.random.default_rng(7).standard_normal((nE, 30))
    st["kiteForCell"][:st.nCells] = 7
    ref = run_oracle(st, ofn)
    got = run_gpu(st, gfn, exact=1)
    bad = compare_states(got, ref, rtol=RTOL_POW, tol_fields=tf or None) if tf else compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
def test_irr_atm_core_init(variant):
    st = state(26, variant).copy()
    st["zgrid"][:st.nCells] = np.linspace(0.0, 30000.0, 27)[None, :]
    ref = run_oracle(st, lambda o: o.atm_core_init())
    got = run_gpu(st, lambda c: T.atm_core_init(c), exact=1)
    tf = {"dss", "exner", "exner_base", "pressure_p", "pressure_base", "uReconstructX", "uReconstructY",
          "uReconstructZ", "uReconstructZonal", "uReconstructMeridional", "meshScalingDel2", "meshScalingDel4"}
    bad = compare_states(got, ref, rtol=RTOL_POW, tol_fields=tf)
    assert not bad, bad[:6]


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
def test_irr_summarize_timestep(L):
    """the reductions over 647 cells / 1935 edges (partly filled last blocks), bit-identical"""
    st = state(L, "random")
    for detailed, global_vel in ((1, 1), (1, 0), (0, 1), (0, 0)):
        ref = O.Oracle(st.copy()).summarize_timestep(detailed, global_vel)
        got = _summary_gpu(st, detailed, global_vel)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (detailed, global_vel)
        ok = np.where(np.isnan(ref), True, (got == ref) & (np.signbit(got) == np.signbit(ref)))
        assert ok.all(), f"summarize {detailed}{global_vel}: {np.nonzero(~ok)[0]} {got[~ok]} vs {ref[~ok]}"


# ------------------------------------------------------------------ 3. reference whole steps
@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("schedule", [0, 1])
def test_irr_srk3(L, variant, schedule):
    """(caught: k_acoustic's specified-zone columns returned before the tail that stores the fused
    damping's ru_p of edges owned through slots >= NF -- "random" has specZoneMaskCell != 0)"""
    st = state(L, variant)
    ref = run_oracle(st, lambda o: o.atm_srk3(720.0, schedule))
    got = run_gpu(st, lambda c: T.atm_srk3(c, 720.0, schedule), exact=1)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, f"srk3 exact: {bad[:6]}"
    got = run_gpu(st, lambda c: T.atm_srk3(c, 720.0, schedule), exact=0)
    report_fast(f"srk3-s{schedule}-{variant}-L{L}", got, ref)
    bad = compare_states(got, ref, rtol=RTOL_STEP)
    assert not bad, f"srk3 fast: {bad[:6]}"


def _five_steps(st, exact, **opts):
    snaps, gens = [], []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("exact", exact)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload(st)
        for _ in range(5):
            T.atm_srk3(ctx, 720.0, 1)
            gens.append(ctx.get_option("stepkeep_gen"))
            ctx.sync()
            got = st.copy()
            ctx.download(got)
            snaps.append(got)
    return snaps, gens


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
def test_irr_steps5(L, variant):
    """five consecutive default-option steps.  Exact mode: each equals the oracle's step bit for
    bit, with stepkeep 1 and 2 set (the kept-step forms do not run in exact mode or under the
    small mesh's default hfuse order -- test_gpu_stepkeep.py's inactive paths -- so the
    generation reads 0 there).  The kept forms themselves (vikeep, a0keep, dynkeep on long
    lists) run on the fast path in the large grids' launch order (hfuse 0): the generation
    reads 1, 2, 2, 2, 2 and every field after every step has the bits of stepkeep 0."""
    st = state(L, variant)
    ref = st.copy()
    o = O.Oracle(ref)
    refs = []
    for _ in range(5):
        o.atm_srk3(720.0, 1)
        refs.append(ref.copy())
    for stepkeep in (1, 2):
        snaps, gens = _five_steps(st, 1, stepkeep=stepkeep)
        assert gens == [0] * 5
        for n in range(5):
            bad = compare_states(snaps[n], refs[n], rtol=0.0)
            assert not bad, f"exact, stepkeep={stepkeep}, step {n + 1}: {bad[:6]}"
    off, gens = _five_steps(st, 0, hfuse=0, stepkeep=0)
    assert gens == [0] * 5
    for stepkeep in (1, 2):
        on, gens = _five_steps(st, 0, hfuse=0, stepkeep=stepkeep)
        assert gens == [1, 2, 2, 2, 2]
        for n in range(5):
            bad = compare_states(on[n], off[n], rtol=0.0)
            assert not bad, f"fast, stepkeep={stepkeep} vs 0, step {n + 1}: {bad[:6]}"


# ------------------------------------------------------------------ 4. fusion options
def slot_owners(st):
    """per edge the slot of the lowest (cell * 16 + slot) listing it (k_prepare's rule, X_eowner);
    -1 for an edge no cell lists"""
    eoc, ne = st.arrays["edgesOnCell"][:st.nCells], st.arrays["nEdgesOnCell"].reshape(-1)[:st.nCells]
    owner = np.full(st.nEdges, 0x7fffffff, np.int64)
    for i in range(eoc.shape[1]):
        e = eoc[:, i]
        on = (i < ne) & (e >= 0) & (e < st.nEdges)
        np.minimum.at(owner, e[on], (np.arange(st.nCells) * 16 + i)[on])
    return np.where(owner == 0x7fffffff, -1, owner % 16)


@pytest.mark.parametrize("L", ENDS, ids=END_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("exact", [0, 1])
def test_irr_copies_by_A(L, variant, exact):
    """option fusecopy in the large grids' launch order (hfuse 0): dyn_tend's A stores ru_save / u_2
    of the edges its cell owns -- here also through slots >= NF (dyn_A_body's CPA tail, bits NF..7
    of X_eown) -- with the bits of the setup kernel's copy, at every edge"""
    st = state(L, variant)
    slots = slot_owners(st)
    assert (slots >= NF).sum() >= 1, "no edge is owned through a slot past NF: choose another seed / order"
    outs = {}
    for fc in (1, 0):
        snaps = []
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("exact", exact)
            ctx.set_option("hfuse", 0)
            ctx.set_option("fusecopy", fc)
            ctx.upload(st)
            for _ in range(2):
                T.atm_srk3(ctx, 720.0, 1)
                ctx.sync()
                got = st.copy()
                ctx.download(got)
                snaps.append(got)
        outs[fc] = snaps
    start = [st, outs[1][0]]
    nE = st.nEdges
    for n in range(2):
        bad = compare_states(outs[1][n], outs[0][n], rtol=0.0)
        assert not bad, f"after {n + 1} step(s): {bad[:6]}"
        for dst, src in (("ru_save", "ru"), ("u_2", "u")):
            a = outs[1][n].arrays[dst]
            assert np.array_equal(a[:nE, :L], start[n].arrays[src][:nE, :L], equal_nan=True), (n, dst)
            assert np.array_equal(a[:nE, L], st.arrays[dst][:nE, L], equal_nan=True), (n, dst, "level L")


@pytest.mark.parametrize("L", ENDS, ids=END_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
def test_irr_fusion_options(L, variant):
    """the body of test_gpu_parity.test_fusedamp_bit_identical on this mesh"""
    st = state(L, variant)
    ref = run_oracle(st, lambda o: (o.atm_srk3(720.0, 0), o.atm_srk3(360.0, 1), o.atm_srk3(360.0, 1)))
    got1, orph = _two_steps_gpu(st, 1, 1)
    bad = compare_states(got1, ref, rtol=0.0)
    assert not bad, f"fusedamp exact vs oracle: {bad[:6]}"
    assert orph == (0 if variant == "mpas0" else 1)
    for graph in (1, 0):
        a, _ = _two_steps_gpu(st, 1, 0, graph)
        b, _ = _two_steps_gpu(st, 0, 0, graph)
        bad = compare_states(a, b, rtol=0.0)
        assert not bad, f"fusedamp fast path vs separate damping (graph={graph}): {bad[:6]}"
    c, _ = _two_steps_gpu(st, 0, 0, 1, fusesetup=1)
    bad = compare_states(c, b, rtol=0.0)
    assert not bad, f"fusesetup alone vs separate launches: {bad[:6]}"
    for hf in (0, 1):
        c, _ = _two_steps_gpu(st, hf, 0, 1, hfuse=1 - hf)
        bad = compare_states(c, b, rtol=0.0)
        assert not bad, f"hfuse={1 - hf}, fusedamp={hf} vs separate launches: {bad[:6]}"
    for ex in (0, 1):
        c, _ = _two_steps_gpu(st, 1, ex, 1, tmedge=0, hfuse=1)
        bad = compare_states(c, b if ex == 0 else ref, rtol=0.0)
        assert not bad, f"hfuse=1, tmedge=0, exact={ex}: {bad[:6]}"
    for opt in ("fusecopy", "vdyn", "defer4"):
        for on in (0, 1):
            for ex in (0, 1):
                fd = 1 if opt == "fusecopy" else 1 - on
                c, _ = _two_steps_gpu(st, fd, ex, 1, **{opt: on})
                bad = compare_states(c, b if ex == 0 else ref, rtol=0.0)
                assert not bad, f"{opt}={on}, exact={ex}: {bad[:6]}"
    c, _ = _two_steps_gpu(st, 1, 0, 1, fusesml=0)
    bad = compare_states(c, b, rtol=0.0)
    assert not bad, f"fusesml=0 vs separate launches: {bad[:6]}"
    for tm in (0, 1):
        c, _ = _two_steps_gpu(st, 1 - tm, 0, 1, tmedge=tm)
        bad = compare_states(c, b, rtol=0.0)
        assert not bad, f"tmedge={tm}, fusedamp={1 - tm} vs separate launches: {bad[:6]}"


# ------------------------------------------------------------------ 5. MPAS solver and dynamics
@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
def test_irr_mpas_solver_tasks(L, variant):
    """physics 1: vert_imp, the acoustic step (both substeps) and recover, as
    test_gpu_parity.test_mpas_vert_imp / _acoustic / _recover"""
    st = state(L, variant)
    ref = run_oracle(st, lambda o: o.mpas_vert_imp_coefs(240.0))
    for exact in (1, 0):
        got = run_gpu_mpas(st, lambda c: T.atm_compute_vert_imp_coefs(c, 240.0), exact)
        bad = compare_states(got, ref, rtol=0.0)
        assert not bad, f"vert_imp exact={exact}: {bad[:6]}"
    sst = state(L, variant, solver=True)
    for small_step in (0, 1):
        ref = run_oracle(sst, lambda o: o.mpas_acoustic_step(240.0, small_step))
        for exact, tol in ((1, 0.0), (0, RTOL_FAST)):
            got = run_gpu_mpas(sst, lambda c: T.atm_advance_acoustic_step_work(c, 240.0, small_step), exact)
            if not exact:
                report_fast(f"mpas_acoustic_s{small_step}-{variant}-L{L}", got, ref)
            bad = compare_states(got, ref, rtol=tol)
            assert not bad, f"acoustic s{small_step} exact={exact}: {bad[:6]}"
    for ns, rk_step in ((2, 0), (3, 2)):
        ref = run_oracle(st, lambda o: o.mpas_recover(ns, rk_step, 240.0))
        got = run_gpu_mpas(st, lambda c: T.atm_recover_large_step_variables_work(c, ns, rk_step, 240.0), 1)
        bad = compare_states(got, ref, rtol=RTOL_POW, tol_fields=POW_FIELDS, zero_slot_excluded=ZERO_SLOT_WRITTEN)
        assert not bad, f"recover {ns} {rk_step}: {bad[:6]}"


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("task", DYN_TASKS, ids=[t[0] for t in DYN_TASKS])
def test_irr_mpas_dyn_task(L, variant, task):
    """physics 2: every task of test_gpu_mpas_dynamics.TASKS"""
    name, ofn, gfn, tol_fields = task
    st = state(L, variant, solver=True)
    ref = run_oracle(st, ofn)
    got = run_gpu_dyn(st, gfn, 1)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, f"{name} exact: {bad[:6]}"
    got.check_zero_slots()
    if tol_fields:
        got = run_gpu_dyn(st, gfn, 0)
        report_fast(f"dyn_{name}-{variant}-L{L}", got, ref, tol_fields)
        bad = compare_states(got, ref, rtol=RTOL_FAST, tol_fields=tol_fields)
        assert not bad, f"{name} fast: {bad[:6]}"


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("physics", [1, 2])
@pytest.mark.parametrize("transport", [0, 1])
def test_irr_mpas_srk3(L, physics, transport):
    """test_gpu_mpas_dynamics' whole-step tolerances: exact value-identical but the pow fields; fast
    RTOL_STEP at 5 and 26 levels and, as that file's test_srk3_level_extremes, RTOL_EXTREME at 63,
    where the synthetic state's fields reach 1e18 within the step and the scans' rounding differences
    grow with them (measured here at L = 63, physics 1: alpha_tri 2.5e-9, gamma_tri 1.2e-9 of the
    field's magnitude; physics 2: every field within 1e-9)"""
    st = state(L, "mpas0", solver=True)
    ref = run_oracle(st, lambda o: o.mpas_srk3(720.0, 1, transport=bool(transport), physics=physics))
    for exact, tol, tf in ((1, RTOL_POW, POW_FIELDS), (0, RTOL_EXTREME if L == 63 else RTOL_STEP, None)):
        got = gpu_tr(st, lambda c: T.atm_srk3(c, 720.0, 1), exact=exact, physics=physics, transport=transport)
        if not exact:
            report_fast(f"mpas_srk3-p{physics}-t{transport}-L{L}", got, ref)
        bad = compare_states(got, ref, rtol=tol, tol_fields=tf, zero_slot_excluded=ZERO_SLOT_WRITTEN)
        assert not bad, f"physics={physics} transport={transport} exact={exact}: {bad[:6]}"


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("exact", [1, 0])
def test_irr_mpas_srk3_transport2(L, exact):
    """transport = 2 inside the step == the step with transport 0, then the three task calls
    (test_gpu_transport_rk3.test_srk3_is_the_composition), bit for bit"""
    st = state(L, "mpas0")
    dt = 720.0

    def composed(c):
        T.atm_srk3(c, dt, 1)
        old = st.copy()
        old["scalars_old"][...] = st["scalars"]
        c.upload(old, names=["scalars_old"])
        T.atm_advance_scalars(c, dt / 3)
        T.atm_advance_scalars(c, dt / 2)
        T.atm_advance_scalars_mono_rk(c, dt)
    got = gpu_tr(st, lambda c: T.atm_srk3(c, dt, 1), exact=exact, physics=2, transport=2)
    ref = gpu_tr(st, composed, exact=exact, physics=2, transport=0)
    assert not np.array_equal(got["scalars"], st["scalars"])
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    assert np.array_equal(got["scalars_old"], st["scalars"])


# ------------------------------------------------------------------ 6. transport
_TR = {}


def tr_state(L, const=None):
    key = (L, const)
    if key not in _TR:
        _TR[key] = transport_state(irregular(), L, DT, const=const)
    return _TR[key]


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
@pytest.mark.parametrize("const", [None, 0.0123])
def test_irr_transport_task(L, const):
    st, vol = tr_state(L, const)
    ref = st.copy()
    O.Oracle(ref).mpas_advance_scalars_mono(DT)
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("physics", 1)
        ctx.set_option("trtile", 1)
        ctx.upload(st)
        assert ctx.get_option("trtile_active") == 0  # (a cell with more than NF edges: no tiles)
        print(f"tredge_active {ctx.get_option('tredge_active')} tredge_irregular {ctx.get_option('tredge_irregular')}")
        T.atm_advance_scalars_mono(ctx, DT)
        ctx.sync()
        ctx.download(got)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    nC = st.nCells
    m_old = np.einsum("ck,cki->i", st["rho_zz_old_split"][:nC, :L] * vol, st["scalars_old"][:nC, :L])
    m_new = np.einsum("ck,cki->i", got["rho_zz"][:nC, :L] * vol, got["scalars"][:nC, :L])
    assert np.allclose(m_new, m_old, rtol=1e-12, atol=0)


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
def test_irr_transport_task_random_ids(L):
    """raw 1-based ids (non-SELF gathers, zero slot), every input synthetic"""
    st = state(L, "random")
    ref = st.copy()
    O.Oracle(ref).mpas_advance_scalars_mono(DT)
    got = gpu_tr(st, lambda c: T.atm_advance_scalars_mono(c, DT))
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("L", LEVELS, ids=L_IDS)
def test_irr_transport_rk3_tasks(L):
    """the unlimited stage and the monotonic task on the stage's fluxes against the NumPy
    restatement (tests/transport_ref.py; test_gpu_transport_rk3's rule, 1e-12 normwise)"""
    st, _ = tr_state(L)
    st = st.copy()
    st["scalars"][...] = st["scalars_old"]
    st, _ = R.advance_scalars(st, DT / 3)
    ref, _ = R.advance_scalars(st, DT / 2)
    got = gpu_tr(st, lambda c: T.atm_advance_scalars(c, DT / 2))
    check_transport_task(got, ref, st, f"atm_advance_scalars L={L}")
    ref = R.advance_scalars_mono_rk(st, DT)
    got = gpu_tr(st, lambda c: T.atm_advance_scalars_mono_rk(c, DT))
    check_transport_task(got, ref, st, f"atm_advance_scalars_mono_rk L={L}")


@pytest.mark.parametrize("variant", ["mesh", "random"])
def test_irr_transport_edge_groups(variant):
    """option tredge (LP 64): k_tr_edge_lds against the direct gathers and the oracle, bit for bit"""
    L = 63
    st = tr_state(L)[0] if variant == "mesh" else state(L, "random")
    ref = st.copy()
    O.Oracle(ref).mpas_advance_scalars_mono(DT)
    outs = {}
    for on in (0, 1):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("physics", 1)
            ctx.set_option("tredge", on)
            ctx.upload(st)
            assert ctx.get_option("tredge_active") == on
            if on:
                print(f"tredge_irregular[{variant}] {ctx.get_option('tredge_irregular')}")
            T.atm_advance_scalars_mono(ctx, DT)
            ctx.sync()
            ctx.download(got)
        outs[on] = got
    bad = compare_states(outs[1], outs[0], rtol=0.0)
    assert not bad, bad[:6]
    bad = compare_states(outs[1], ref, rtol=0.0)
    assert not bad, bad[:6]


# ------------------------------------------------------------------ 7. etile
@pytest.mark.parametrize("variant", ["random", "mpas0"])
def test_irr_etile_inactive(variant):
    """tiles_build refuses a cell with more than NF edges: etile 1 runs the untiled E, the same bits
    as etile 0 (fast and exact), and exact equals the oracle"""
    st = state(63, variant)
    ref = run_oracle(st, lambda o: o.atm_srk3(720.0, 1))
    outs = {}
    for exact in (0, 1):
        for etile in (0, 1):
            got = st.copy()
            with lib.Context(*st.dims()) as ctx:
                ctx.set_option("exact", exact)
                ctx.set_option("etile", etile)
                ctx.upload(st)
                T.atm_srk3(ctx, 720.0, 1)
                ctx.sync()
                assert ctx.get_option("etile_active") == 0
                ctx.download(got)
            outs[(exact, etile)] = got
        bad = compare_states(outs[(exact, 1)], outs[(exact, 0)], rtol=0.0)
        assert not bad, f"exact={exact}: {bad[:6]}"
    for etile in (0, 1):
        bad = compare_states(outs[(1, etile)], ref, rtol=0.0)
        assert not bad, f"etile={etile} vs oracle: {bad[:6]}"


# ------------------------------------------------------------------ 8. decomposition
@pytest.mark.parametrize("L", ENDS, ids=END_IDS)
@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_irr_srk3_decomposed(L, variant, nparts, overlap):
    st = state(L, variant)
    step = lambda c: T.atm_srk3(c, 720.0, 1)  # noqa: E731
    for exact in (1, 0):
        ref = run_single(st, step, exact)
        got, stats = run_decomposed(st, nparts, step, exact, overlap=overlap)
        bad = compare_states(got, ref, rtol=0.0)
        assert not bad, f"exact={exact}: {bad[:6]}"
        assert all(s[0] > 0 for s in stats)


@pytest.mark.parametrize("L", ENDS, ids=END_IDS)
@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_irr_mpas_srk3_decomposed(L, nparts, overlap):
    """physics 2 with the transport inside the step"""
    st = state(L, "mpas0", solver=True)

    def step(c):
        c.set_option("physics", 2)
        c.set_option("transport", 1)
        T.atm_srk3(c, 720.0, 1)
    for exact in (1, 0):
        ref = run_single(st, step, exact)
        got, stats = run_decomposed(st, nparts, step, exact, overlap=overlap)
        bad = compare_states(got, ref, rtol=0.0)
        assert not bad, f"exact={exact}: {bad[:6]}"
        assert all(s[0] > 0 for s in stats)


@pytest.mark.parametrize("task", ["dyn_tend_rk0", "dyn_tend_rk1", "solve_holl", "acoustic", "div_damp", "smlstep",
                                  "recover", "reconstruct"])
def test_irr_task_decomposed(task):
    fn = {"dyn_tend_rk0": lambda c: T.atm_compute_dyn_tend_work(c, 0, 720.0),
          "dyn_tend_rk1": lambda c: T.atm_compute_dyn_tend_work(c, 1, 720.0),
          "solve_holl": lambda c: T.atm_compute_solve_diagnostics(c, True, -1),
          "acoustic": lambda c: T.atm_advance_acoustic_step_work(c, 360.0, 1),
          "div_damp": lambda c: T.atm_divergence_damping_3d(c, 240.0),
          "smlstep": lambda c: T.atm_set_smlstep_pert_variables_work(c),
          "recover": lambda c: T.atm_recover_large_step_variables_work(c, 2, 2, 240.0),
          "reconstruct": lambda c: T.mpas_reconstruct_2d(c, False, True)}[task]
    st = state(63, "random")
    ref = run_single(st, fn, 1)
    for overlap in (1, 0):
        got, _ = run_decomposed(st, 3, fn, 1, overlap=overlap)
        bad = compare_states(got, ref, rtol=0.0)
        assert not bad, (overlap, bad[:6])
