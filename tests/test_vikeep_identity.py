"""The premise of option `vikeep`, on the CPU oracle alone.

Every input of atm_compute_vert_imp_coefs is a field no task of the reference-semantics step writes (zz, exner,
theta_m, cqw, qtot, the base fields, rtheta_p), so each of the step's two coefficient sets -- stage 0's, formed
with dts = dt / 3 after the setup and the moist coefficients, and stage 1's, dts = dt / 2 -- is the same bytes in
every consecutive step, but for alpha_tri and gamma_tri: Q17's recurrence reads the gamma_tri the call found.
Those two follow from the stored a_tri, b_tri, c_tri and that gamma_tri by

    alpha(k) = 1.0 / (b(k) - a(k) * gamma_old(k-1)),  gamma_old(0) = 0;  gamma(k) = c(k) * alpha(k),  0 < k < L

bit for bit, which is what the kept launches evaluate.  And h_divergence, stage 2's kernel A's one output, is the
same bytes after every step.
"""
import numpy as np
import pytest

import oracle as O
from helpers import make_state

DT = 720.0
SET = ("cofwt", "cofwz", "cofwr", "coftz", "a_tri", "b_tri", "c_tri")


def _alpha_gamma(a, b, c, gamma_old, n, L):
    """the two expressions on rows 0 .. n-1, levels 1 .. L-1"""
    g_m = gamma_old[:n, 0:L - 1].copy()
    g_m[:, 0] = 0.0  # (gamma(0) was just zeroed by the call)
    alpha = 1.0 / (b[:n, 1:L] - a[:n, 1:L] * g_m)
    return alpha, c[:n, 1:L] * alpha


def _stage0_set(st):
    """stage 0's set on the state a step left: the three tasks the step's first launch stands for"""
    tw = st.copy()
    gamma_old = tw["gamma_tri"].copy()
    o = O.Oracle(tw)
    o.atm_rk_integration_setup()
    o.atm_compute_moist_coefficients()
    o.atm_compute_vert_imp_coefs(DT / 3)
    return tw, gamma_old


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_vert_imp_sets_are_kept(x1_2562, L, variant):
    st = make_state(x1_2562, L, variant)
    n = st.dims()[0]
    o = O.Oracle(st)
    sets0, hdiv, ends = [], [], []
    for step in range(4):  # (the start of steps 1 .. 4: step 1's set, then the one each step's end gives)
        tw, gamma_old = _stage0_set(st)
        sets0.append({f: tw[f].tobytes() for f in SET})
        with np.errstate(all="ignore"):
            alpha, gamma = _alpha_gamma(tw["a_tri"], tw["b_tri"], tw["c_tri"], gamma_old, n, L)
        assert alpha.tobytes() == tw["alpha_tri"][:n, 1:L].tobytes()
        assert gamma.tobytes() == tw["gamma_tri"][:n, 1:L].tobytes()
        if step == 3:
            break
        o.atm_srk3(DT, 1)
        ends.append(st.copy())
        hdiv.append(st["h_divergence"].tobytes())
    assert sets0[0] == sets0[1] == sets0[2] == sets0[3]
    assert hdiv[0] == hdiv[1] == hdiv[2]
    # stage 1's set, as each step's end holds it: the same bytes too, and another set than stage 0's
    for f in SET:
        assert ends[0][f].tobytes() == ends[1][f].tobytes() == ends[2][f].tobytes(), f
    assert all(ends[2][f].tobytes() != sets0[2][f] for f in ("cofwt", "cofwz", "a_tri", "b_tri", "c_tri"))


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_stage1_alpha_gamma_from_stored_abc(x1_2562, L, variant):
    """stage 1's call, replayed on a twin: its alpha_tri / gamma_tri follow from the a, b, c the step's end holds
    and the gamma_tri the call found"""
    st = make_state(x1_2562, L, variant)
    n = st.dims()[0]
    o = O.Oracle(st)
    for _ in range(3):
        o.atm_srk3(DT, 1)
        tw = st.copy()
        gamma_old = tw["gamma_tri"].copy()
        O.Oracle(tw).atm_compute_vert_imp_coefs(DT / 2)
        for f in SET:  # (the call stores what the fields hold)
            assert tw[f].tobytes() == st[f].tobytes(), f
        with np.errstate(all="ignore"):
            alpha, gamma = _alpha_gamma(st["a_tri"], st["b_tri"], st["c_tri"], gamma_old, n, L)
        assert alpha.tobytes() == tw["alpha_tri"][:n, 1:L].tobytes()
        assert gamma.tobytes() == tw["gamma_tri"][:n, 1:L].tobytes()
