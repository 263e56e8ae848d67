// N-step returns (include/dqnx.h "n-step returns"): "nstep_gather", the first compute launch of every
// learn step of an n-step engine.  It runs once the step's physical slot table is final (after the
// sampler launch, or after the previous step's copy of a minibatch drawn ahead) and materialises the
// minibatch the step's other launches read in place of the replay ring:
//
//   mb_obs[b]  = ring_obs[slot(p_b)]                         (+ the bf16 copy where the engine keeps one)
//   mb_next[b] = ring_next_obs[slot(last_b)]                 (+ the bf16 copy)
//   mb_act[b], mb_rew[b] = (float)R, mb_done[b] = d, mb_disc[b] = fp32(gamma^m)      (nstep.hpp)
//   mb_phys[b] = b                                           the identity slot table of those rows
//   mb_start[b] = {act, rew, done, 0} of the START row       (what the statistics launch describes)
//
// Shape: one workgroup = one 16-row tile x one column part; 16 lanes per row, each moving up to
// kNstepPieces 16-byte pieces of the row per matrix.  A row costs two memory round trips behind the slot
// table: (1) the n (rew, done) scalars of the window -- their addresses depend on the start slot only,
// so they issue together and the window is resolved in registers -- beside the obs row's pieces,
// (2) the next_obs row's pieces at `last`.  Every lane group of a row folds the window itself (the
// scalar loads of its 16 lanes coalesce); part 0 writes the row's scalars.  No atomics, no LDS, no
// barrier; bad ring state is reported through dqnx_ctrl.error and the row falls back to a one-position
// window at a clamped slot, so every address stays inside the ring.
//
// Placement (speed only): on the fused MLP plan the workgroups of tile t run on the XCD that runs row
// tile t of the forward launch (the rule k_head_bwd uses), so the forward gathers rows its own XCD's L2
// holds.
#include <algorithm>

#include "common.hpp"
#include "learn.hpp"
#include "nstep.hpp"

namespace dqnx {

namespace {

template <int NMAX, bool BF>
__global__ __launch_bounds__(kNstepThreads) void k_nstep_gather(NstepArgs a) {
    const int tid = threadIdx.x;
    const int r = tid >> 4, l16 = tid & 15;
    int tile = (int)blockIdx.x;
    const int part = (int)blockIdx.y;
    if (a.xcd_rows) {   // tile t on the XCD of the forward's row tile t / xcd_mr (tiles % (8 * xcd_mr) == 0)
        const int msh = __builtin_ctz(a.xcd_mr);
        const int xh = tile & 7, k = tile >> 3;
        tile = ((((k >> msh) * 8 + ((xh - a.xcd_shift) & 7))) << msh) + (k - ((k >> msh) << msh));
    }
    if (tile >= a.tiles) return;
    const int b = tile * 16 + r;
    const bool valid = b < a.Bl;
    const int bc = valid ? b : a.Bl - 1;
    const int64_t cap = a.capacity;
    const int64_t size = gld(&a.ctrl->ring_size), wptr = gld(&a.ctrl->ring_wptr);
    const int32_t s0 = gld(a.phys + bc);

    // the start row's logical position p = (slot - (wptr - size)) mod capacity, checked against the ring
    bool bad = size < 1 || size > cap || wptr < 0 || wptr >= cap || s0 < 0 || s0 >= cap;
    const int64_t slot0 = s0 < 0 ? 0 : (s0 >= cap ? cap - 1 : (int64_t)s0);
    int64_t base = wptr - size;
    if (base < 0) base += cap;
    int64_t p = slot0 - base;
    if (p < 0) p += cap;
    if (bad || p >= size) {
        bad = true;
        p = 0;
    }
    const int nv = bad ? 1 : nstep_positions(size, p, a.n_step, a.n_env);

    // (1) the window's scalars: clamped positions past the window re-read its last one
    float rw[NMAX], dn[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; j++) {
        const int jc = j < nv ? j : nv - 1;
        int64_t sj = slot0 + (int64_t)jc * a.n_env;   // (offset < size <= capacity: one wrap at most)
        if (sj >= cap) sj -= cap;
        rw[j] = gld(a.ring_rew + sj);
        dn[j] = gld(a.ring_done + sj);
    }
    const int32_t act0 = gld(a.ring_act + slot0);

    //     ... beside the obs row's pieces
    const int q4 = a.stride >> 2, q8 = a.stride16 >> 3;
    const int c0 = part * kNstepChunk + l16;
    u32x4 xo[kNstepPieces], xn[kNstepPieces];
    u32x4 ho[BF ? kNstepPieces : 1], hn[BF ? kNstepPieces : 1];
    {
        const float* src = a.ring_obs + slot0 * a.stride;
#pragma unroll
        for (int k = 0; k < kNstepPieces; k++) {
            const int c = c0 + 16 * k;
            xo[k] = __builtin_bit_cast(u32x4, ld4(src + 4 * (c < q4 ? c : 0)));
        }
        if constexpr (BF) {
            const uint16_t* src16 = a.ring16_obs + slot0 * a.stride16;
#pragma unroll
            for (int k = 0; k < kNstepPieces; k++) {
                const int c = c0 + 16 * k;
                ho[k] = *reinterpret_cast<const u32x4*>(src16 + 8 * (c < q8 ? c : 0));
            }
        }
    }

    float R, d, disc;
    int m;
    nstep_fold<NMAX>(rw, dn, nv, a.gamma, &R, &d, &disc, &m);
    int64_t last = slot0 + (int64_t)(m - 1) * a.n_env;
    if (last >= cap) last -= cap;

    // (2) the next_obs row at `last`
    {
        const float* src = a.ring_next + last * a.stride;
#pragma unroll
        for (int k = 0; k < kNstepPieces; k++) {
            const int c = c0 + 16 * k;
            xn[k] = __builtin_bit_cast(u32x4, ld4(src + 4 * (c < q4 ? c : 0)));
        }
        if constexpr (BF) {
            const uint16_t* src16 = a.ring16_next + last * a.stride16;
#pragma unroll
            for (int k = 0; k < kNstepPieces; k++) {
                const int c = c0 + 16 * k;
                hn[k] = *reinterpret_cast<const u32x4*>(src16 + 8 * (c < q8 ? c : 0));
            }
        }
    }

    if (bad && l16 == 0 && part == 0) *(volatile int32_t*)&a.ctrl->error = DQNX_DEVERR_NSTEP_STATE;
    if (!valid) return;
    if (part == 0 && l16 == 0) {
        a.mb_act[b] = act0;
        a.mb_rew[b] = R;
        a.mb_done[b] = d;
        a.mb_disc[b] = disc;
        a.mb_phys[b] = b;
        a.mb_start[b] = make_float4(__int_as_float(act0), rw[0], dn[0], 0.f);
    }
    {
        float* dst = a.mb_obs + (int64_t)b * a.stride;
#pragma unroll
        for (int k = 0; k < kNstepPieces; k++) {
            const int c = c0 + 16 * k;
            if (c < q4) *reinterpret_cast<u32x4*>(dst + 4 * c) = xo[k];
        }
        if constexpr (BF) {
            uint16_t* dst16 = a.mb16_obs + (int64_t)b * a.stride16;
#pragma unroll
            for (int k = 0; k < kNstepPieces; k++) {
                const int c = c0 + 16 * k;
                if (c < q8) *reinterpret_cast<u32x4*>(dst16 + 8 * c) = ho[k];
            }
        }
    }
    {
        float* dst = a.mb_next + (int64_t)b * a.stride;
#pragma unroll
        for (int k = 0; k < kNstepPieces; k++) {
            const int c = c0 + 16 * k;
            if (c < q4) *reinterpret_cast<u32x4*>(dst + 4 * c) = xn[k];
        }
        if constexpr (BF) {
            uint16_t* dst16 = a.mb16_next + (int64_t)b * a.stride16;
#pragma unroll
            for (int k = 0; k < kNstepPieces; k++) {
                const int c = c0 + 16 * k;
                if (c < q8) *reinterpret_cast<u32x4*>(dst16 + 8 * c) = hn[k];
            }
        }
    }
}

template <int NMAX>
int launch_n(const NstepArgs& a, dim3 grid, hipStream_t s) {
    if (a.stride16) DQNX_LAUNCH((k_nstep_gather<NMAX, true>), grid, dim3(kNstepThreads), 0, s, a);
    else DQNX_LAUNCH((k_nstep_gather<NMAX, false>), grid, dim3(kNstepThreads), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace

int nstep_parts(int stride) { return std::max(1, ((stride >> 2) + kNstepChunk - 1) / kNstepChunk); }

int launch_nstep_gather(const NstepArgs& a, hipStream_t s) {
    if (!a.ctrl || !a.phys || !a.ring_obs || !a.ring_next || !a.ring_act || !a.ring_rew || !a.ring_done || !a.mb_obs ||
        !a.mb_next || !a.mb_act || !a.mb_rew || !a.mb_done || !a.mb_disc || !a.mb_phys || !a.mb_start)
        return set_error(DQNX_EINVAL, "nstep gather: null buffer");
    if (a.stride16 && (!a.ring16_obs || !a.ring16_next || !a.mb16_obs || !a.mb16_next))
        return set_error(DQNX_EINVAL, "nstep gather: null bf16 buffer");
    if (a.Bl < 1 || a.n_step < 1 || a.n_step > DQNX_NSTEP_MAX || a.n_env < 1 || a.capacity < 1 || a.stride < 4 ||
        a.stride % 4 || a.stride16 % 8 || a.stride16 > 2 * a.stride)
        return set_error(DQNX_EINVAL, "nstep gather: bad shape");
    if (a.tiles != (a.Bl + 15) / 16 || a.parts != nstep_parts(a.stride))
        return set_error(DQNX_EINVAL, "nstep gather: the grid does not cover the minibatch");
    if (a.xcd_rows && !((a.xcd_mr == 1 || a.xcd_mr == 2 || a.xcd_mr == 4) && a.tiles % (8 * a.xcd_mr) == 0 &&
                        a.xcd_shift >= 0 && a.xcd_shift <= 7))
        return set_error(DQNX_EINVAL, "nstep gather: XCD row mapping needs tiles %% (8 * mr) == 0");
    const uintptr_t al = (uintptr_t)a.ring_obs | (uintptr_t)a.ring_next | (uintptr_t)a.mb_obs | (uintptr_t)a.mb_next |
                         (uintptr_t)a.ring16_obs | (uintptr_t)a.ring16_next | (uintptr_t)a.mb16_obs |
                         (uintptr_t)a.mb16_next | (uintptr_t)a.mb_start;
    if (al & 15) return set_error(DQNX_EINVAL, "nstep gather: misaligned buffer");
    const dim3 grid((unsigned)a.tiles, (unsigned)a.parts);
    if (a.n_step <= 1) return launch_n<1>(a, grid, s);
    if (a.n_step <= 2) return launch_n<2>(a, grid, s);
    if (a.n_step <= 4) return launch_n<4>(a, grid, s);
    if (a.n_step <= 8) return launch_n<8>(a, grid, s);
    return launch_n<16>(a, grid, s);
}

}  // namespace dqnx
