"""NumPy restatement of the sigma-level statistics task, mpas_atm_sigma_stats_accumulate
(include/mpas_dyn.h; kernel: mpas-regent_amd/csrc/k_stats.hip).  The authority for the task: its
formulas in the kernel's operand order, every operation an IEEE double one, so the sample count and
the ps column are the kernel's bit for bit and every other accumulator differs by the device's log
alone.  The logs of the targets are libm's, taken per target as the library takes them on the host at
configure time.  Pinned on the CPU by tests/test_sigma_stats.py."""
import math

import numpy as np

from forcing_ref import surface_pressure

STATS = ("n", "u", "v", "T", "uu", "vv", "TT", "uv", "vT")
DEFAULT_SIGMA = tuple(round(0.975 - 0.05 * j, 3) for j in range(20))


def decreasing_pressures(st, seed=1234):
    """overwrite st's pressures for the synthetic test cases: pressure_base a positive profile that
    decreases with the level, 1e5 exp(-5 (k + jitter) / L) with a jitter of up to 0.3 levels per cell and
    level, and pressure_p its raw random value scaled under 1 % of it"""
    nC, L = st.nCells, st.L
    rng = np.random.default_rng(seed + L)
    k = np.arange(L)[None, :]
    pb = 1.0e5 * np.exp(-(k + 0.3 * (2.0 * rng.random((nC, L)) - 1.0)) * (5.0 / L))
    st["pressure_p"][:nC, :L] = 0.009 * pb * (st["pressure_p"][:nC, :L] / 500.0)
    st["pressure_base"][:nC, :L] = pb
    return st


def new_acc(nCells, nsigma):
    acc = {name: np.zeros((nCells, nsigma)) for name in STATS}
    acc["ps"] = np.zeros((nCells, 3))
    return acc


def columns(st):
    """the task's inputs per owned cell and level k < L: dict(ps [nC], s, ls, u, v, T [nC, L])"""
    nC, L = st.nCells, st.L
    p = st["pressure_base"][:nC, :L] + st["pressure_p"][:nC, :L]
    ps = surface_pressure(st)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = p / ps[:, None]
        ls = np.log(s)
    return {"ps": ps, "s": s, "ls": ls, "u": st["uReconstructZonal"][:nC, :L].copy(),
            "v": st["uReconstructMeridional"][:nC, :L].copy(), "T": st["theta_m"][:nC, :L] * st["exner"][:nC, :L]}


def brackets(s, sigma):
    """kb [nC, nsigma]: the lowest k in 0..L-2 with s(k) >= sigma_j > s(k+1), -1 where there is none;
    decided on s itself (a NaN compares false, as on the device)"""
    sg = np.asarray(sigma, dtype=np.float64)
    nC, L = s.shape
    if L < 2:
        return np.full((nC, len(sg)), -1)
    with np.errstate(invalid="ignore"):
        q = (s[:, :-1, None] >= sg[None, None, :]) & (sg[None, None, :] > s[:, 1:, None])
    return np.where(q.any(axis=1), q.argmax(axis=1), -1)


def sample(st, sigma, cols=None):
    """one sample: dict(kb, hit [nC, nsigma], u, v, T [nC, nsigma] (garbage where not hit), ps [nC])"""
    d = columns(st) if cols is None else cols
    lsig = np.array([math.log(x) for x in sigma])
    kb = brackets(d["s"], sigma)
    hit = kb >= 0
    k0 = np.where(hit, kb, 0)
    k1 = np.minimum(k0 + 1, d["s"].shape[1] - 1)
    take = lambda x, k: np.take_along_axis(x, k, axis=1)  # noqa: E731
    out = {"kb": kb, "hit": hit, "ps": d["ps"]}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l0 = take(d["ls"], k0)
        a = (lsig[None, :] - l0) / (take(d["ls"], k1) - l0)
        for name in ("u", "v", "T"):
            x0 = take(d[name], k0)
            out[name] = x0 + a * (take(d[name], k1) - x0)
    out["a"] = a
    return out


def accumulate(acc, st, sigma, cols=None):
    """the task: one sample of st added to acc (new_acc), plain `acc += x`; returns the sample"""
    smp = sample(st, sigma, cols)
    hit = smp["hit"]
    U, V, T = smp["u"], smp["v"], smp["T"]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = {"n": np.ones_like(U), "u": U, "v": V, "T": T, "uu": U * U, "vv": V * V, "TT": T * T, "uv": U * V,
                 "vT": V * T}
    for name in STATS:
        acc[name] += np.where(hit, terms[name], 0.0)
    ps = smp["ps"]
    acc["ps"][:, 0] += ps
    acc["ps"][:, 1] += ps * ps
    acc["ps"][:, 2] += 1.0
    return smp
