// k_stats.hip -- time-mean statistics on sigma levels for gfx950 (the Held-Suarez climate): one sample of
// every owned cell column, interpolated to the configured sigma targets and added to per-cell fp64
// accumulators of the first and second moments.  No reference task exists; the formulas are stated in
// include/mpas_dyn.h (mpas_atm_sigma_stats_accumulate) and restated in NumPy, in this operand order, by
// tests/stats_ref.py.
// Same column mapping as the rest of the library: one wavefront per cell column (LP = 64; 64 / LP columns
// below it), lane = level.  Every input is the cell's own column: no gather, no halo.  A translation unit
// of its own: no kernel of the step is compiled with it.
#include "mpas_dev.h"

namespace mpas {

// One cell column.  Eight own columns in four paired 16-B loads; ps is k_hs_cells' expression (k_forcing.hip),
// term for term.  The column's s = p / ps, log s (the kernel's one libm call, once per model level), u, v and
// T = theta_m exner are staged in LDS; lane j (then j + LP, ...) takes target sigma_j, scans s itself -- never
// its logarithm -- for the lowest bracket kb in 0..L-2 with s(kb) >= sigma_j > s(kb+1), interpolates linearly in
// log s and adds the nine moments to its slots of the cell's record with plain read-add-write: every slot has
// one writer and the order is call order, so two runs give the same bits.  A pair with no bracket adds 0.0
// (the accumulators are never -0.0, so the sum is the slot's own bits): the record is rewritten as a whole.
// The padding lanes and level L hold values no bracket reaches (kb + 1 <= L - 1).
template <int LP>
__global__ __launch_bounds__(256) void k_sigma_stats(DevState S, double* __restrict__ acc,
                                                     const double* __restrict__ sig, int ns, int rec) {
    __shared__ double sh_s[256], sh_l[256], sh_u[256], sh_v[256], sh_t[256];
    ColMap<LP> m(S, KC);
    const int L = S.L, k = m.k;
    const bool own = m.ent < S.nCO;  // (no early return: the block meets at the barrier below)
    const int c = own ? m.ent : S.nCO - 1;
    const double dz0 = 1.0 / ldc(fd(S, F_rdzw));
    double pb, pp, rz, q, tm, ex, u, v;
    gather2<LP>(fd(S, F_pressure_base), c, fd(S, F_pressure_p), c, k, pb, pp);
    gather2<LP>(fd(S, F_rho_zz), c, fd(S, F_qtot), c, k, rz, q);
    gather2<LP>(fd(S, F_theta_m), c, fd(S, F_exner), c, k, tm, ex);
    gather2<LP>(fd(S, F_uReconstructZonal), c, fd(S, F_uReconstructMeridional), c, k, u, v);
    const double rq = rz * (1.0 + q), rq1 = lvl_up<LP>(rq, k);
    const double ps = __shfl(0.5 * dz0 * kGravity * (1.25 * rq - 0.25 * rq1) + pp + pb, 0, LP);
    const double p = pb + pp;
    const double s = p / ps;
    const int t = (int)threadIdx.x, t0 = t - k;  // t0: the column's first LDS slot
    sh_s[t] = s;
    sh_l[t] = log(s);
    sh_u[t] = u;
    sh_v[t] = v;
    sh_t[t] = tm * ex;
    __syncthreads();
    double* r = acc + (size_t)c * (size_t)rec;
    for (int j = k; j < ns; j += LP) {
        const double sg = sig[j], lg = sig[kStatsMaxSigma + j];
        int kb = -1;
        double s0 = sh_s[t0];
        for (int kk = 0; kk + 1 < L; kk++) {  // (wave-uniform trip count; every lane reads the same slot)
            const double s1 = sh_s[t0 + kk + 1];
            kb = (kb < 0 && s0 >= sg && sg > s1) ? kk : kb;
            s0 = s1;
        }
        const bool hit = kb >= 0;
        const int a0 = t0 + (hit ? kb : 0), a1 = a0 + 1;  // (LP >= 8: slot 1 exists at L = 1)
        const double l0 = sh_l[a0];
        const double a = (lg - l0) / (sh_l[a1] - l0);
        const double u0 = sh_u[a0], v0 = sh_v[a0], x0 = sh_t[a0];
        const double U = u0 + a * (sh_u[a1] - u0);
        const double V = v0 + a * (sh_v[a1] - v0);
        const double T = x0 + a * (sh_t[a1] - x0);
        if (own) {
            double* rj = r + j;
            rj[0 * ns] += hit ? 1.0 : 0.0;
            rj[1 * ns] += hit ? U : 0.0;
            rj[2 * ns] += hit ? V : 0.0;
            rj[3 * ns] += hit ? T : 0.0;
            rj[4 * ns] += hit ? U * U : 0.0;
            rj[5 * ns] += hit ? V * V : 0.0;
            rj[6 * ns] += hit ? T * T : 0.0;
            rj[7 * ns] += hit ? U * V : 0.0;
            rj[8 * ns] += hit ? V * T : 0.0;
        }
    }
    if (own && k < 3) r[kStatsMoments * ns + k] += k == 0 ? ps : k == 1 ? ps * ps : 1.0;
}

template <int LP>
static hipError_t sigma_stats_lp(const DevState& S, hipStream_t st, double* acc, const double* sig, int ns) {
    const int ncb = col_blocks<LP>(S, KC);
    if (ncb) k_sigma_stats<LP><<<ncb, 256, 0, st>>>(S, acc, sig, ns, stats_rec(ns));
    return hipGetLastError();
}
hipError_t launch_sigma_stats(const DevState& S, hipStream_t st, double* acc, const double* sig, int nsigma) {
    if (!acc || !sig || nsigma < 1 || nsigma > kStatsMaxSigma) return hipErrorInvalidValue;
    MPAS_LP_DISPATCH(S.LP, sigma_stats_lp, S, st, acc, sig, nsigma);
}

}  // namespace mpas
