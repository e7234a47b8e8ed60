// k_forcing.hip -- the Held-Suarez (1994) forcing for gfx950: the first producer of the physics
// tendencies the MPAS forms of dyn_tend read (physics = 2).  No reference task exists; the formulas
// are stated in include/mpas_dyn.h (mpas_atm_held_suarez_forcing) and restated in NumPy, in this
// operand order, by tests/forcing_ref.py.
//   cells   tend_rtheta_physics = -kT rho_zz (theta_m - theta_eq): Newtonian relaxation to the
//           radiative equilibrium, as a potential temperature (divided through by exner)
//   edges   tend_ru_physics = -(0.5 (kv(cell1) + kv(cell2))) ru: Rayleigh friction below sigma_b
// Same column mapping as the rest of the library: one wavefront per cell / edge column, lane =
// level.  A translation unit of its own: no kernel of the step is compiled with it.
#include "mpas_dev.h"
#include "mpas_halo.h"

namespace mpas {

// One cell column.  Six own columns in three paired 16-B loads; the surface pressure is
// k_output_diag's expression (physics = 2, k_diag.hip) formed by every lane from its levels k and
// k + 1 and taken from lane 0, so it reads level 1 of rho_zz and qtot as found (level L at L = 1).
// Stored: tend_rtheta_physics (level L its kept value, the padding zeros: every line whole) and,
// for the edge kernel, the friction rate kv in the scratch column X_hskv (zeros from level L up).
template <int LP>
__global__ __launch_bounds__(256) void k_hs_cells(DevState S) {
    ColMap<LP> m(S, KC);
    const int L = S.L, k = m.k, c = m.ent;
    if (c >= S.nCO) return;
    const double cl = ldc(fd(S, X_cosLatCell) + c);
    const double dz0 = 1.0 / ldc(fd(S, F_rdzw));
    const double kl = keepv<LP>(S, F_tend_rtheta_physics, KC, c);
    double pb, pp, rz, q, tm, ex;
    gather2<LP>(fd(S, F_pressure_base), c, fd(S, F_pressure_p), c, k, pb, pp);  // (every lane: gather2)
    gather2<LP>(fd(S, F_rho_zz), c, fd(S, F_qtot), c, k, rz, q);
    gather2<LP>(fd(S, F_theta_m), c, fd(S, F_exner), c, k, tm, ex);
    const double rq = rz * (1.0 + q), rq1 = lvl_up<LP>(rq, k);
    const double ps = __shfl(0.5 * dz0 * kGravity * (1.25 * rq - 0.25 * rq1) + pp + pb, 0, LP);
    const double c2 = cl * cl;
    const double p = pb + pp;
    const double sigma = p / ps;
    const double x = (sigma - kHsSigmaB) / (1.0 - kHsSigmaB);
    const double w = x > 0.0 ? x : 0.0;
    const double kv = kHsKf * w;
    const double kT = kHsKa + (kHsKs - kHsKa) * w * c2 * c2;
    const double tfl = kHsFloor / ex;
    const double trd = 315.0 - kHsDeltaTy * (1.0 - c2) - kHsDeltaThz * log(p / kP0) * c2;
    const double theq = tfl > trd ? tfl : trd;
    const double tend = -kT * rz * (tm - theq);
    // (the padding lanes hold 0 / ps and log(0): never stored)
    put2f<LP>(fw(S, F_tend_rtheta_physics), c, fw(S, X_hskv), c, k, KEEPW(tend, kl), k < L ? kv : 0.0);
}

// Two consecutive edge columns per slot (as the other few-gather kernels: the loads of both are
// issued before the first store): ru, and kv at the two cells of the edge in one paired gather
template <int LP>
__global__ __launch_bounds__(256) void k_hs_edges(DevState S) {
    constexpr int EPW = 2;
    ColMapN<LP, EPW> m(S, KE);
    const int L = S.L, k = m.k;
    const int* coe = fi(S, F_cellsOnEdge);
    const double *ru_f = fd(S, F_ru), *kv_f = fd(S, X_hskv);
    int c1[EPW], c2[EPW];
    double ru[EPW], kv1[EPW], kv2[EPW], kl[EPW];
#pragma unroll
    for (int i = 0; i < EPW; i++) {
        const int e = min(m.base + i, S.nEO - 1);
        c1[i] = ldc(coe + (size_t)e * 2);
        c2[i] = ldc(coe + (size_t)e * 2 + 1);
        kl[i] = keepv<LP>(S, F_tend_ru_physics, KE, e);
        ru[i] = colk(ru_f, e);
    }
#pragma unroll
    for (int i = 0; i < EPW; i++) gather2s<LP>(kv_f, c1[i], c2[i], k, kv1[i], kv2[i]);
#pragma unroll
    for (int i = 0; i < EPW; i++) {
        const int e = m.base + i;
        if (e >= S.nEO) break;  // (wave-uniform at LP = 64; below it a per-column store mask)
        colk(fw(S, F_tend_ru_physics), e) = KEEPW(-(0.5 * (kv1[i] + kv2[i])) * ru[i], kl[i]);
    }
}

template <int LP>
static hipError_t held_suarez_lp(const DevState& S, hipStream_t st) {
    const int ncb = col_blocks<LP>(S, KC);
    if (ncb) k_hs_cells<LP><<<ncb, 256, 0, st>>>(S);
    HALO_WROTE(S, F_tend_rtheta_physics, X_hskv);
    // decomposed: kv at the ghost cells of the owned edges comes by an exchange of the scratch
    auto run = [&](const DevState& X) {
        const int nb = col_blocks_n<LP, 2>(X, KE);
        if (nb) k_hs_edges<LP><<<nb, 256, 0, st>>>(X);
    };
    HALO_RUN(S, st, run, X_hskv);
    HALO_WROTE(S, F_tend_ru_physics);
    return hipGetLastError();
}
hipError_t launch_held_suarez_forcing(const DevState& S, hipStream_t st) {
    MPAS_LP_DISPATCH(S.LP, held_suarez_lp, S, st);
}

}  // namespace mpas
