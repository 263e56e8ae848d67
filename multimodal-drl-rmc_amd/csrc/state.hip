// State restore (dqnx_state_load): the bf16 copies of the replay rows of a bf16 engine, regenerated
// from the restored fp32 rows.  The push kernel writes both copies of a row it stores
// (k_replay_push, learn.hip); a restored ring arrives as fp32 rows only, so this kernel -- used on
// that path alone -- makes the bf16 ones: the same rounding (RNE, bf16_bits) of the same fp32 values,
// pad columns zero.
#include "common.hpp"
#include "learn.hpp"

namespace dqnx {

// One wave per ring row, 4 rows per workgroup; blockIdx.y = 0: obs, 1: next_obs.  Lane t converts the
// 8-element groups t, t + 64, ...: two 16-byte loads of the fp32 row, one 16-byte store of the bf16 row.
// The fp32 rows are `stride` floats (a multiple of 4, >= obs_dim) on 16-byte boundaries, the bf16 rows
// `stride16` elements (obs_dim rounded up to 8): a float4 is loaded only where it lies inside the row.
__global__ __launch_bounds__(256) void k_ring16_rebuild(Ring16Args a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const float* src = (blockIdx.y ? a.ring_next : a.ring_obs) + row * a.stride;
    uint16_t* dst = (blockIdx.y ? a.ring16_next : a.ring16_obs) + row * a.stride16;
    for (int g = lane; g * 8 < a.stride16; g += 64) {
        const int j = g * 8;
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (j + 4 <= a.stride) lo = ld4(src + j);
        if (j + 8 <= a.stride) hi = ld4(src + j + 4);
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t b0 = j + 2 * u < a.obs_dim ? bf16_bits(v[2 * u]) : 0u;
            const uint32_t b1 = j + 2 * u + 1 < a.obs_dim ? bf16_bits(v[2 * u + 1]) : 0u;
            w[u] = b0 | (b1 << 16);
        }
        u32x4 o;
        o.x = w[0];
        o.y = w[1];
        o.z = w[2];
        o.w = w[3];
        *reinterpret_cast<u32x4*>(dst + j) = o;
    }
}

int launch_ring16_rebuild(const Ring16Args& a, hipStream_t s) {
    if (a.rows <= 0) return DQNX_OK;
    if (!a.ring_obs || !a.ring_next || !a.ring16_obs || !a.ring16_next)
        return set_error(DQNX_EINVAL, "ring16 rebuild: null ring");
    if (a.stride % 4 || a.stride16 % 8 || a.stride < a.obs_dim || a.stride16 < a.obs_dim || a.obs_dim <= 0 ||
        (((uintptr_t)a.ring_obs | (uintptr_t)a.ring_next | (uintptr_t)a.ring16_obs | (uintptr_t)a.ring16_next) & 15))
        return set_error(DQNX_EINVAL, "ring16 rebuild: row geometry");
    if (a.rows > a.capacity || (a.rows + 3) / 4 > 0x7fffffffll) return set_error(DQNX_EINVAL, "ring16 rebuild: rows");
    DQNX_LAUNCH(k_ring16_rebuild, dim3((unsigned)((a.rows + 3) / 4), 2), dim3(256), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
