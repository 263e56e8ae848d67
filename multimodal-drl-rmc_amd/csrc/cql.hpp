// Conservative Q-learning, CQL(H) for discrete actions (include/dqnx.h "conservative Q-learning"): the
// per-element forms of the regulariser, shared by the two head kernels (fused.hip k_head_bwd<.., CQL = true>,
// one lane per action slot; learn.hip k_head<.., CQL = true>, one thread per row through cql_row) and the
// host test hook (dqnx_cql_row, engine.cpp), so that all of them fold the same expressions.
//
// Per sampled row, from the fp32 Q_online(s, .) after the dueling aggregate, a = the clamped replay action:
//
//   m    = max_j q_j
//   e_j  = expf(q_j - m)          (libm-grade expf / logf, never the fast intrinsics)
//   s    = sum_j e_j              (the kernels may sum in different orders)
//   gap  = (m + logf(s)) - q_a    = logsumexp_j q_j - q_a  >= 0 up to rounding
//   p_j  = e_j / s
//   dq_j = gq * [j == a] + cb * (p_j - [j == a]),   cb = fp32(alpha) * inv_bg
//
// gq is the TD gradient of q_a (Huber, IS-weighted under PER); the regulariser itself is never
// importance-weighted.  The row's loss contribution becomes lb + fp32(alpha) * gap.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dqnx.h"

namespace dqnx {

__host__ __device__ inline float cql_exp(float q, float m) { return expf(q - m); }

__host__ __device__ inline float cql_gap(float m, float s, float qa) {
    const float lse = m + logf(s);
    return lse - qa;
}

// p_j - [j == a]
__host__ __device__ inline float cql_pm(float e, float s, bool hit) {
    const float p = e / s;
    return p - (hit ? 1.f : 0.f);
}

// dq_j from the TD gradient and the regulariser's share
__host__ __device__ inline float cql_dq(float gq, float cb, float pm, bool hit) {
    const float t = cb * pm;
    return (hit ? gq : 0.f) + t;
}

__host__ __device__ inline float cql_loss(float lb, float alpha, float gap) {
    const float t = alpha * gap;
    return lb + t;
}

// One row, serially: q[0 .. A) (A = 1 .. 16), act already clamped into [0, A).  Writes gap and
// pm[j] = p_j - [j == act] for j < A.  A == 1: e = s = 1, so gap == 0 and pm[0] == 0 exactly.
__host__ __device__ inline void cql_row(const float* q, int A, int act, float* gap, float* pm) {
    float m = q[0];
    for (int j = 1; j < A; j++) m = fmaxf(m, q[j]);
    float s = 0.f;
    for (int j = 0; j < A; j++) {   // e_j parked in the output row (no indexed private array on the device)
        const float e = cql_exp(q[j], m);
        pm[j] = e;
        s += e;
    }
    *gap = cql_gap(m, s, q[act]);
    for (int j = 0; j < A; j++) pm[j] = cql_pm(pm[j], s, j == act);
}

}  // namespace dqnx
