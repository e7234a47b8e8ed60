// k_pbl.hip -- bulk surface fluxes and implicit boundary-layer mixing for gfx950: the surface-flux and boundary-
// layer part of the simple-physics package of Reed & Jablonowski (2012) over an ocean of prescribed temperature,
// on the model's own layers and layer mass (the source works on pressure thicknesses) and with the mixing ratio qv
// where the source has specific humidity.  No reference task exists; the formulas are stated in include/mpas_dyn.h
// (mpas_atm_surface_pbl) and restated in NumPy, in this operand order, by tests/pbl_ref.py.
//   cells   theta_m, rtheta_p, exner, pressure_p and scalar 0 (qv): time-split state updates like Kessler's; the
//           momentum change as a tendency per cell, Fu and Fv, in the scratch columns X_pblFu / X_pblFv
//   edges   tend_ru_physics = 0.5 (Fu(c1) + Fu(c2)) cosA + 0.5 (Fv(c1) + Fv(c2)) sinA: the cell-centre vector
//           projected onto the edge normal, as MPAS-A projects its boundary-layer wind tendencies
// Same column mapping as the rest of the library: one wavefront per cell / edge column (LP = 64; 64 / LP columns
// below it), lane = level.  A translation unit of its own: no kernel of the step is compiled with it.
#include "mpas_dev.h"
#include "mpas_halo.h"

namespace mpas {

// One cell column.  Twelve own columns in six paired 16-B loads, the cell's scalar pair 0 (qv, scalar 1) in one
// 16-B load; the surface pressure is the forcing task's expression (k_forcing.hip) formed by every lane and taken
// from lane 0, the level below / above by lane shuffles inside the column's LP lanes.  The two tridiagonal systems
// -- momentum (u, v) and heat (theta, qv), each with its two right-hand sides on one elimination -- are a
// nonlinear recurrence over the levels: as vert_imp's (k_cols.h vi_column), the block's columns run it side by
// side, one lane per (column, system), on coefficients staged in LDS, in the restatement's order, instead of
// every lane of a column's wavefront stepping through all L levels; nothing of it crosses a column.  Every wave
// of the block reaches both barriers (no early return: a column past the owned cells is clamped and not stored).
// The levels from L up compute on stand-in values and store what they hold (level L of a keep field its kept
// value, the padding zeros, the scalar pair as loaded): every line whole.
template <int LP>
__global__ __launch_bounds__(256) void k_pbl_cells(DevState S, double dt, const double* __restrict__ sst,
                                                   double* __restrict__ sflux) {
    ColMap<LP> m(S, KC);
    const int L = S.L, k = m.k;
    const bool own = m.ent < S.nCO;
    const int c = own ? m.ent : S.nCO - 1;
    const bool lv = k < L;
    auto kL = [&](int f) { return keepv<LP>(S, f, KC, c); };
    const double kl_tm = kL(F_theta_m), kl_rtp = kL(F_rtheta_p), kl_ex = kL(F_exner), kl_pp = kL(F_pressure_p);
    const double Ts = ldc(sst + c);
    const double dz0 = 1.0 / ldc(fd(S, F_rdzw));
    double pb, pp, rz, qt, tm, ex, rtp, zz, rtb, exb, ua, va;
    gather2<LP>(fd(S, F_pressure_base), c, fd(S, F_pressure_p), c, k, pb, pp);
    gather2<LP>(fd(S, F_rho_zz), c, fd(S, F_qtot), c, k, rz, qt);
    gather2<LP>(fd(S, F_theta_m), c, fd(S, F_exner), c, k, tm, ex);
    gather2<LP>(fd(S, F_rtheta_p), c, fd(S, F_zz), c, k, rtp, zz);
    gather2<LP>(fd(S, F_rtheta_base), c, fd(S, F_exner_base), c, k, rtb, exb);
    gather2<LP>(fd(S, F_uReconstructZonal), c, fd(S, F_uReconstructMeridional), c, k, ua, va);
    double2* sc = (double2*)fw(S, F_scalars) + (size_t)(uint32_t)c * (kPairW / 2) * LP + k;
    double2* p0 = (double2*)MPAS_CHK(fd(S, F_scalars), sc, 16);
    const double2 s01 = *p0;
    double rdzw = fd(S, F_rdzw)[k];
    // ps: lane 0's, from levels 0 and 1 of rho_zz and qtot as found (level L at L = 1)
    const double rq = rz * (1.0 + qt), rq1 = lvl_up<LP>(rq, k);
    const double ps = __shfl(0.5 * dz0 * kGravity * (1.25 * rq - 0.25 * rq1) + pp + pb, 0, LP);
    // the levels from L up: stand-ins that keep the arithmetic finite; nothing of them is stored or used below L
    if (!lv) pb = kP0, pp = 0.0, tm = 300.0, rz = 1.0, zz = 1.0, ex = 1.0, rdzw = 1.0, ua = 0.0, va = 0.0;
    const double qv = lv ? s01.x : 0.0;

    const double rvord = kKsRv / kRgas;
    const double ms = rz / rdzw;
    const double dz = 1.0 / (rdzw * zz);
    const double rho_d = zz * rz;
    const double p = pb + pp;
    const double pi = ex;
    const double theta = tm / (1.0 + rvord * qv);
    const double za = 0.5 * __shfl(dz, 0, LP);
    const double ua0 = __shfl(ua, 0, LP), va0 = __shfl(va, 0, LP);
    const double wind = sqrt(ua0 * ua0 + va0 * va0);
    const double cd = wind < kPblWindSw ? kPblCd0 + kPblCd1 * wind : kPblCdMax;
    const double qss = kPblEps / ps * kPblE0 * exp(-kPblLvRv * (1.0 / Ts - 1.0 / kPblT00));
    const double am = cd * wind * dt / za;
    const double ah = kPblCh * wind * dt / za;
    // the surface step: level 0 only
    const bool k0 = k == 0;
    const double u1 = k0 ? ua / (1.0 + am) : ua;
    const double v1 = k0 ? va / (1.0 + am) : va;
    const double th1 = k0 ? (theta + ah * Ts / pi) / (1.0 + ah) : theta;
    const double q1 = k0 ? (qv + ah * qss) / (1.0 + ah) : qv;
    const double E = ms * (q1 - qv);  // (lane 0's is the column's)
    // the mixing coefficient at the interface below level k (between k - 1 and k), 0 at k = 0 and from L up
    const double dzm = lvl_dn<LP>(dz, k), pm = lvl_dn<LP>(p, k), rdm = lvl_dn<LP>(rho_d, k);
    const double s = dz + dzm;
    const double pint = (dz * pm + dzm * p) / s;
    const double rhoi = (dz * rdm + dzm * rho_d) / s;
    const double dzc = 0.5 * s;
    const double xf = (kPblPTop - pint) / kPblPDecay;
    const double f = pint >= kPblPTop ? 1.0 : exp(-(xf * xf));
    const bool intf = k >= 1 && lv;
    const double Dm = intf ? rhoi * cd * wind * za * f / dzc : 0.0;
    const double Dh = intf ? rhoi * kPblCh * wind * za * f / dzc : 0.0;
    const double Dm_u = lvl_up<LP>(Dm, k), Dh_u = lvl_up<LP>(Dh, k);
    const double a_m = -dt * Dm / ms, c_m = -dt * Dm_u / ms, b_m = 1.0 - a_m - c_m;
    const double a_h = -dt * Dh / ms, c_h = -dt * Dh_u / ms, b_h = 1.0 - a_h - c_h;

    // the Thomas algorithm, tests/pbl_ref.py thomas(): per (column, system) one lane, level by level
    constexpr int CPB = 256 / LP;
    __shared__ double s_a[2][CPB][LP + 1], s_b[2][CPB][LP + 1], s_c[2][CPB][LP + 1], s_x[2][CPB][LP + 1],
        s_y[2][CPB][LP + 1];
    const int j = (int)(threadIdx.x / LP);
    s_a[0][j][k] = a_m, s_b[0][j][k] = b_m, s_c[0][j][k] = c_m, s_x[0][j][k] = u1, s_y[0][j][k] = v1;
    s_a[1][j][k] = a_h, s_b[1][j][k] = b_h, s_c[1][j][k] = c_h, s_x[1][j][k] = th1, s_y[1][j][k] = q1;
    __syncthreads();
    if ((int)threadIdx.x < 2 * CPB) {
        const int sy = (int)threadIdx.x / CPB, jj = (int)threadIdx.x % CPB;
        double *A = s_a[sy][jj], *B = s_b[sy][jj], *C = s_c[sy][jj], *X = s_x[sy][jj], *Y = s_y[sy][jj];
        // (loading the next level's operands ahead of this level's arithmetic was measured and gave nothing: the
        // loop is bound by the dependent chain through the reciprocal, not by the LDS round trips)
        double cp = 0.0, xp = 0.0, yp = 0.0;
        for (int kk = 0; kk < L; kk++) {
            const double a = A[kk];
            const double al = 1.0 / (B[kk] - a * cp);
            cp = C[kk] * al;
            xp = (X[kk] - a * xp) * al;
            yp = (Y[kk] - a * yp) * al;
            C[kk] = cp;
            X[kk] = xp;
            Y[kk] = yp;
        }
        for (int kk = L - 2; kk >= 0; kk--) {
            const double g = C[kk];
            xp = X[kk] - g * xp;
            yp = Y[kk] - g * yp;
            X[kk] = xp;
            Y[kk] = yp;
        }
    }
    __syncthreads();
    const double u2 = s_x[0][j][k], v2 = s_y[0][j][k], th2 = s_x[1][j][k], q2 = s_y[1][j][k];

    // Kessler's increment forms and recover's two expressions (MPAS form)
    const double dth = th2 - theta;
    const double tm1 = tm + dth * (1.0 + rvord * q2) + theta * rvord * (q2 - qv);
    const double dtm = tm1 - tm;
    const double rtp1 = rtp + rz * dtm;
    const double ex1 = pow(zz * (kRgas / kP0) * (rtp1 + rtb), kRgas / (kCp - kRgas));
    const double pp1 = zz * kRgas * (ex1 * rtp1 + rtb * (ex1 - exb));
    const double Fu = rz * (u2 - ua) / dt, Fv = rz * (v2 - va) / dt;
    if (!own) return;
    put2f<LP>(fw(S, F_theta_m), c, fw(S, F_rtheta_p), c, k, KEEPW(tm1, kl_tm), KEEPW(rtp1, kl_rtp));
    put2f<LP>(fw(S, F_exner), c, fw(S, F_pressure_p), c, k, KEEPW(ex1, kl_ex), KEEPW(pp1, kl_pp));
    put2f<LP>(fw(S, X_pblFu), c, fw(S, X_pblFv), c, k, lv ? Fu : 0.0, lv ? Fv : 0.0);
    *p0 = lv ? make_double2(q2, s01.y) : s01;
    if (k == 0) {  // one writer per slot, plain read-add-write in call order: two runs give the same bits
        const size_t nC = (size_t)S.nCells;
        sflux[c] += E;
        sflux[nC + c] = E;
        sflux[2 * nC + c] += 1.0;
    }
}

// Two consecutive edge columns per slot (as k_hs_edges: the loads of both are issued before the first store): Fu
// and Fv at the two cells of the edge in one paired gather each
template <int LP>
__global__ __launch_bounds__(256) void k_pbl_edges(DevState S) {
    constexpr int EPW = 2;
    ColMapN<LP, EPW> m(S, KE);
    const int L = S.L, k = m.k;
    const int* coe = fi(S, F_cellsOnEdge);
    const double *fu_f = fd(S, X_pblFu), *fv_f = fd(S, X_pblFv);
    int c1[EPW], c2[EPW];
    double cosA[EPW], sinA[EPW], fu1[EPW], fu2[EPW], fv1[EPW], fv2[EPW], kl[EPW];
#pragma unroll
    for (int i = 0; i < EPW; i++) {
        const int e = min(m.base + i, S.nEO - 1);
        c1[i] = ldc(coe + (size_t)e * 2);
        c2[i] = ldc(coe + (size_t)e * 2 + 1);
        cosA[i] = ldc(fd(S, X_cosAngleEdge) + e);
        sinA[i] = ldc(fd(S, X_sinAngleEdge) + e);
        kl[i] = keepv<LP>(S, F_tend_ru_physics, KE, e);
    }
#pragma unroll
    for (int i = 0; i < EPW; i++) {
        gather2s<LP>(fu_f, c1[i], c2[i], k, fu1[i], fu2[i]);
        gather2s<LP>(fv_f, c1[i], c2[i], k, fv1[i], fv2[i]);
    }
#pragma unroll
    for (int i = 0; i < EPW; i++) {
        const int e = m.base + i;
        if (e >= S.nEO) break;  // (wave-uniform at LP = 64; below it a per-column store mask)
        const double t = 0.5 * (fu1[i] + fu2[i]) * cosA[i] + 0.5 * (fv1[i] + fv2[i]) * sinA[i];
        colk(fw(S, F_tend_ru_physics), e) = KEEPW(t, kl[i]);
    }
}

template <int LP>
static hipError_t surface_pbl_lp(const DevState& S, hipStream_t st, double dt, const double* sst, double* sflux) {
    const int ncb = col_blocks<LP>(S, KC);
    if (ncb) k_pbl_cells<LP><<<ncb, 256, 0, st>>>(S, dt, sst, sflux);
    // owned cells only, every input the cell's own: no gather; the ghosts of what it wrote are stale
    HALO_WROTE(S, F_theta_m, F_rtheta_p, F_exner, F_pressure_p, F_scalars, X_pblFu, X_pblFv);
    // decomposed: Fu, Fv at the ghost cells of the owned edges come by an exchange of the scratch
    auto run = [&](const DevState& X) {
        const int nb = col_blocks_n<LP, 2>(X, KE);
        if (nb) k_pbl_edges<LP><<<nb, 256, 0, st>>>(X);
    };
    HALO_RUN(S, st, run, X_pblFu, X_pblFv);
    HALO_WROTE(S, F_tend_ru_physics);
    return hipGetLastError();
}
hipError_t launch_surface_pbl(const DevState& S, hipStream_t st, double dt, const double* sst, double* sflux) {
    if (!sst || !sflux) return hipErrorInvalidValue;
    MPAS_LP_DISPATCH(S.LP, surface_pbl_lp, S, st, dt, sst, sflux);
}

}  // namespace mpas
