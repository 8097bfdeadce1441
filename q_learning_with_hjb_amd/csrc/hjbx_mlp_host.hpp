// hjbx_mlp_host.hpp -- host code every launcher of the two matrix-core kernels shares (hjbx_mlp.hip, hjbx_softpd.hip, and hjbx_user.hip for a
// user-defined system): the normalisation constants as the kernels take them, and the persistent grids.  Not part of the ABI.
#pragma once
#include "hjbx_host.hpp"
#include "hjbx_mlp_kernels.hpp"

// mean, 1/std, xf and eps_scalar of a network descriptor, rounded to float once per call
template <int N> inline MlpP<N> make_mlp_params(const double* mean, const double* std, const double* xf, double eps_scalar) {
    MlpP<N> p;
    for (int k = 0; k < N; ++k) { p.mean[k] = (float)mean[k]; p.istd[k] = (float)(1.0 / std[k]); p.xf[k] = (float)xf[k]; }
    p.eps_s = (float)eps_scalar;
    return p;
}

// value gradient: tile groups of 32 * TL environments; one resident workgroup per CU (106 KB of LDS each); small batches are spread one
// tile group per CU rather than packed eight to a workgroup, so up to n_cu matrix pipes work on them
inline int mlp_value_grad_grid(int64_t B, int TL, int64_t* ngroups, int64_t* grid, const char* who) {
    *ngroups = (B + 32 * TL - 1) / (32 * TL);
    const int n_cu = hjbx_device_cus();
    if (n_cu <= 0) return hjbx_set_error(HJBX_ENODEVICE, "%s: no HIP device", who);
    *grid = *ngroups < n_cu ? *ngroups : n_cu;
    return HJBX_OK;
}

// rollout: as above with one tile per wave, plus the schedule and the test hook for workgroups that cannot be resident before others finish
inline int mlp_rollout_grid(int64_t B, int64_t* ngroups, int64_t* grid, int* sched, const char* who) {
    if (int rc = mlp_value_grad_grid(B, 1, ngroups, grid, who)) return rc;
    *sched = hjbx_option_value(HJBX_OPT_ROLLOUT_SCHEDULE);
    *grid += hjbx_option_value(HJBX_OPT_ROLLOUT_EXTRA_WORKGROUPS);
    if (*grid > kMaxGrid) *grid = kMaxGrid;
    return HJBX_OK;
}
