"""The premise of option `a0keep`, on the CPU oracle alone.

Stage 0's dyn_tend kernel A stores tend_rho, dpdz, the setup copies ru_save / u_2 and the Smagorinsky kdiff (and
h_divergence, where it is live).  All but kdiff are functions of fields no task of the reference-semantics step
writes, so they are one set of bytes after every step.  kdiff reads v, and stage 2 of the first step replaces the
uploaded v with the reconstructed one: kdiff after step 2 differs from kdiff after step 1, and is fixed from then
on -- it is what an rk_step 0 dyn_tend alone stores on the state step 1 left.  The stock test states hide this:
their kdiff sits at its cap everywhere.  With u and v scaled by 1e-6 it is below the cap nearly everywhere.
And ruAvg has no writer in the reference semantics, so the finish's edge copy ruAvg_split = ruAvg is the
identity from the second consecutive step on.
"""
import numpy as np
import pytest

import oracle as O
from helpers import SCRATCH, make_state
from mpasdyn.registry import FIELDS

DT = 720.0
WIND = 1e-6
EVOLVING = {"rho_pp", "rtheta_pp", "rtheta_pp_old", "ru_p", "rw_p", "wwAvg", "wwAvg_split", "alpha_tri", "gamma_tri",
            "tend_u", "w"}
FIXED = ("tend_rho", "dpdz", "ru_save", "u_2", "h_divergence", "ruAvg", "ruAvg_split")
CAP = 0.01 * 120000.0 * 120000.0 / DT  # (k_dyn.hip make_dynk: 0.01 len_disp^2 / dt = 200000.0)


def scaled_state(mesh, L, variant):
    """the stock state with u and v scaled so that the Smagorinsky kdiff leaves its cap"""
    st = make_state(mesh, L, variant)
    st["u"][...] *= WIND
    st["v"][...] *= WIND
    return st


def _differ(a, b):
    return {f.name for f in FIELDS if f.name not in SCRATCH and a[f.name].tobytes() != b[f.name].tobytes()}


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_kdiff_and_the_kept_stores(x1_2562, L, variant):
    st = scaled_state(x1_2562, L, variant)
    n = st.dims()[0]
    o = O.Oracle(st)
    ends = []
    for _ in range(3):
        o.atm_srk3(DT, 1)
        ends.append(st.copy())
    kd = [e["kdiff"] for e in ends]
    # fixed from step 2 on ...
    assert kd[1].tobytes() == kd[2].tobytes()
    # ... but step 1's is another one, nearly everywhere (so none of this is vacuous), below the cap
    with np.errstate(invalid="ignore"):
        moved = kd[0][:n, :L] != kd[1][:n, :L]
    frac = float(np.mean(moved))
    print("kdiff differs between steps 1 and 2 at", frac, "of the points; below the cap at",
          float(np.mean(kd[1][:n, :L] < CAP)))
    assert frac >= 0.90
    # what an rk_step 0 dyn_tend alone stores on the state step 1 left
    tw = ends[0].copy()
    O.Oracle(tw).atm_compute_dyn_tend_work(0, DT)
    assert tw["kdiff"].tobytes() == kd[1].tobytes()
    # kernel A's other stores, and the finish's edge copy: one set of bytes
    for f in FIXED:
        assert ends[0][f].tobytes() == ends[1][f].tobytes() == ends[2][f].tobytes(), f
    L_ = st.L  # (the finish copies every level but L, which keeps the uploaded value in both)
    assert ends[2]["ruAvg_split"][:, :L_].tobytes() == ends[2]["ruAvg"][:, :L_].tobytes()
    d23 = _differ(ends[1], ends[2])
    assert d23 <= EVOLVING | {"w_2"}, sorted(d23 - EVOLVING - {"w_2"})
    assert "kdiff" in _differ(ends[0], ends[1])
