"""The premise of option `stepkeep`, on the CPU oracle alone.

The reference-semantics step never calls recover (Q7), so no task of atm_srk3 writes u, ru, rw, rho_zz,
theta_m, rho_p, rtheta_p, h, zz, exner, the base fields or the reconstructed winds, and every dyn_tend
call zeroes w below level L and forms it again.  Most of what a step stores is therefore a function of
fields no step changes:

* from the third consecutive step on, only the EVOLVING set differs between one step's end and the
  next's -- the acoustic state, the Q17 recurrence's alpha_tri / gamma_tri, tend_u, and w at level L;
* between the ends of steps 1 and 2 the four FIRST fields differ too (and w_2): stage 0's dyn_tend of
  step 1 reads the uploaded diagnostics, that of step 2 the ones the step formed itself;
* a perturbation of every evolving field on its owned rows, at every level, reaches only the evolving
  set and w_2 (the setup's copy of w) in the step that follows: no kept field depends on them.
"""
import numpy as np
import pytest

import oracle as O
from helpers import SCRATCH, make_state
from mpasdyn.registry import FIELDS

EVOLVING = {"rho_pp", "rtheta_pp", "rtheta_pp_old", "ru_p", "rw_p", "wwAvg", "wwAvg_split", "alpha_tri", "gamma_tri",
            "tend_u", "w"}
FIRST = {"delsq_divergence", "delsq_u", "delsq_vorticity", "tend_u_euler", "w_2"}
ACOUSTIC = {"rho_pp", "rtheta_pp", "ru_p", "rw_p"}
DT = 720.0


def _differ(a, b):
    """the fields whose bytes differ between two states (the reference's per-task scratch aside)"""
    return {f.name for f in FIELDS if f.name not in SCRATCH and a[f.name].tobytes() != b[f.name].tobytes()}


def _w_differs_at_level_L_alone(a, b):
    L = a.L
    return a["w"][:, :L].tobytes() == b["w"][:, :L].tobytes()


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_evolving_set(x1_2562, L, variant):
    st = make_state(x1_2562, L, variant)
    o = O.Oracle(st)
    ends = []
    for _ in range(3):
        o.atm_srk3(DT, 1)
        ends.append(st.copy())
    d12, d23 = _differ(ends[0], ends[1]), _differ(ends[1], ends[2])
    assert d23 <= EVOLVING, sorted(d23 - EVOLVING)
    assert d12 <= EVOLVING | FIRST, sorted(d12 - EVOLVING - FIRST)
    assert _w_differs_at_level_L_alone(ends[0], ends[1]) and _w_differs_at_level_L_alone(ends[1], ends[2])
    # (not vacuous: the acoustic state did move, in both intervals)
    assert ACOUSTIC <= d12 and ACOUSTIC <= d23, (sorted(d12), sorted(d23))


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_no_kept_field_depends_on_the_evolving_set(x1_2562, L, variant):
    st = make_state(x1_2562, L, variant)
    o = O.Oracle(st)
    for _ in range(2):
        o.atm_srk3(DT, 1)
    twin = st.copy()
    rng = np.random.default_rng(4711)
    by_name = {f.name: f for f in FIELDS}
    for name in sorted(EVOLVING):
        a = twin[name]
        n = twin.n_of(by_name[name])  # (the owned rows: the zero slot, row n, stays 0.0)
        fin = np.where(np.isfinite(a[:n]), a[:n], 0.0)
        scale = float(np.max(np.abs(fin))) or 1.0
        a[:n] = fin * (1.0 + 0.01 * rng.standard_normal(fin.shape)) + 1e-3 * scale * rng.standard_normal(fin.shape)
        assert a[:n].tobytes() != st[name][:n].tobytes()
    o.atm_srk3(DT, 1)
    O.Oracle(twin).atm_srk3(DT, 1)
    d = _differ(st, twin)
    assert d <= EVOLVING | {"w_2"}, sorted(d - EVOLVING - {"w_2"})
    assert _w_differs_at_level_L_alone(st, twin)
    assert ACOUSTIC <= d, sorted(d)  # (the perturbation did reach the step)
