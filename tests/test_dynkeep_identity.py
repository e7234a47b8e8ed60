"""The premise of option `dynkeep`, on the CPU oracle alone.

In the reference semantics no task of atm_srk3 writes the fields dyn_tend reads but w at level L (which its edge
section reads for tend_u) and tend_u_euler (which stage 0 forms and a later stage reads).  From the second
consecutive step on, everything the three dyn_tend calls of a step store -- tend_u aside -- is therefore what the
same call of the step before stored: the state right after stage s's dyn_tend of step n and of step n + 1 differ in
the evolving set alone, and w below level L is one set of bytes.  Between steps 1 and 2 that does not hold (stage 0
of step 1 reads the uploaded diagnostics and v, step 2 the ones step 1 formed), which the states with u and v scaled
by 1e-6 show in w below level L and in tend_u_euler nearly everywhere: the columns a kept step reuses have to come
from a kept step, not from the full one.

The step is replayed task by task through the oracle's own task calls (ora_atm_srk3's sequence), so that the
state can be looked at after each stage's dyn_tend; the replay equals atm_srk3 byte for byte after every step.
"""
import numpy as np
import pytest

import oracle as O
from helpers import make_state
from mpasdyn.registry import FIELDS
from test_a0keep_identity import scaled_state

DT = 720.0
EVOLVING = {"rho_pp", "rtheta_pp", "rtheta_pp_old", "rw_p", "wwAvg", "wwAvg_split", "ru_p", "alpha_tri", "gamma_tri",
            "tend_u", "w", "w_2"}
STEPS = 4


def replay_step(o, dt, snaps):
    """ora_atm_srk3(dt, 1) as its task calls; a copy of the state after each stage's dyn_tend goes to snaps"""
    sub = (dt / 3, dt / 2, dt / 2)
    nsub = (1, 1, 2)
    o.atm_rk_integration_setup()
    o.atm_compute_moist_coefficients()
    o.atm_compute_vert_imp_coefs(sub[0])
    for rk in range(3):
        if rk == 1:
            o.atm_compute_vert_imp_coefs(sub[rk])
        o.atm_compute_dyn_tend_work(rk, dt)
        snaps.append(o.state.copy())
        o.atm_set_smlstep_pert_variables_work()
        for small in range(nsub[rk] + 1):
            o.atm_advance_acoustic_step_work(sub[rk], small)
            o.atm_divergence_damping_3d(sub[rk])
        o.atm_compute_solve_diagnostics(0, rk)
    o.atm_rk_dynamics_substep_finish(1, 1)


def _differ(a, b):
    return {f.name for f in FIELDS if a[f.name].tobytes() != b[f.name].tobytes()}


def _state(mesh, L, variant, wind):
    return scaled_state(mesh, L, variant) if wind != 1.0 else make_state(mesh, L, variant)


@pytest.mark.parametrize("wind", [1.0, 1e-6])
@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_dyn_tend_stores_what_the_step_before_stored(x1_2562, L, variant, wind):
    st = _state(x1_2562, L, variant, wind)
    twin = st.copy()
    o, ot = O.Oracle(st), O.Oracle(twin)
    after = []  # after[step][stage]: the state right after that dyn_tend call
    for n in range(STEPS):
        snaps = []
        replay_step(o, DT, snaps)
        ot.atm_srk3(DT, 1)
        assert not _differ(st, twin), (n + 1, sorted(_differ(st, twin)))
        after.append(snaps)
    for n in (1, 2):  # steps 2 / 3 and 3 / 4
        for s in range(3):
            a, b = after[n][s], after[n + 1][s]
            d = _differ(a, b)
            assert d <= EVOLVING, (n + 1, s, sorted(d - EVOLVING))
            assert a["w"][:, :L].tobytes() == b["w"][:, :L].tobytes(), (n + 1, s)
    if wind != 1.0:  # (not vacuous: the full step's columns are not the kept steps')
        nC, nE = st.dims()[0], st.dims()[1]
        a, b = after[0][0], after[1][0]
        with np.errstate(invalid="ignore"):
            fw = float(np.mean(a["w"][:nC, :L] != b["w"][:nC, :L]))
            ft = float(np.mean(a["tend_u_euler"][:nE, :L] != b["tend_u_euler"][:nE, :L]))
        print("after stage 0's dyn_tend of steps 1 and 2: w below L differs at", fw, "of the points, tend_u_euler at", ft)
        assert fw > 0.0
        assert ft >= 0.90
