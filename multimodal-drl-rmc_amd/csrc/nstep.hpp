// N-step returns (include/dqnx.h "n-step returns"): the window arithmetic, shared by the device kernel
// (nstep.hip, k_nstep_gather) and the host test hook (dqnx_nstep_window, engine.cpp) so that both fold
// the same expression tree.
//
// A push of n_env rows is one time step, so the successor of logical replay position p in the same
// environment is p + n_env.  The window of a sampled start row p is positions p, p + n_env, ... cut by
// the first done != 0 or by the newest end of the ring:
//
//   g = 1; R = 0; m = 0; d = 0                    (fp64)
//   for j in 0 .. n-1:
//       q = p + j * n_env;  if q >= size: break
//       R += g * (double)rew[q]                    one fp64 multiply, one fp64 add, never contracted
//       g *= gamma                                 repeated multiply, not pow
//       m = j + 1
//       if done[q] != 0: d = 1; break
//   row = (obs[p], act[p], (float)R, d, next_obs[p + (m - 1) * n_env]),  disc = (float)g = fp32(gamma^m)
//
// m >= 1 always; n = 1 gives R = rew[p], d = done[p] (0 / 1 in the ring), disc = (float)gamma.
#pragma once
#include <stdint.h>

#include "../../include/dqnx.h"

namespace dqnx {

// window positions inside the ring: the j in [0, n) with p + j * n_env < size (p < size: at least 1)
__host__ __device__ inline int nstep_positions(int64_t size, int64_t p, int n, int n_env) {
    const int64_t fit = (size - 1 - p) / n_env + 1;
    return fit < (int64_t)n ? (int)fit : n;
}

// The fold over a window whose scalars are already loaded: rw[j] / dn[j] = reward / done of window
// position j, read for j < nv only (nv = nstep_positions, 1 .. NMAX).  A fixed trip count with
// predicates instead of early exits: fully unrolled, rw / dn stay in registers on the device.
template <int NMAX>
__host__ __device__ inline void nstep_fold(const float (&rw)[NMAX], const float (&dn)[NMAX], int nv, double gamma,
                                           float* R, float* d, float* disc, int* m) {
#pragma clang fp contract(off)
    double g = 1.0, acc = 0.0;
    float dd = 0.f;
    int mm = 0;
    bool open = true;
#pragma unroll
    for (int j = 0; j < NMAX; j++) {
        if (open && j < nv) {
            const double t = g * (double)rw[j];
            acc = acc + t;
            g = g * gamma;
            mm = j + 1;
            if (dn[j] != 0.f) {
                dd = 1.f;
                open = false;
            }
        }
    }
    *R = (float)acc;
    *d = dd;
    *disc = (float)g;
    *m = mm;
}

}  // namespace dqnx
