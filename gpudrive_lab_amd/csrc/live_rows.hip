// gd_live_rows: a byte mask [n] to the ascending list of the indices whose byte is not zero, and its length, on the device.
// Two launches over blocks of GD_LIVE_ROWS_BLOCK = 1024 rows (256 lanes, four consecutive rows to a lane):
//   k_live_count   scratch[block] = the block's rows with a set byte
//   k_live_write   every block adds up scratch[0 .. block) for its first position, scans its own 1024 rows (a lane's four, a
//                  shuffle scan over the wave, the four waves through LDS) and stores its indices in order; the last lane of
//                  the last block stores the total to *count, and to *count_copy when the caller keeps a record of it
// No atomics: a position is a sum of integers, so equal input gives equal bytes.  rows[*count .. n) is not written.
// ZERO instantiates both kernels for the complement, the rows whose byte IS zero (gd_bc_rollout_compact lists dead[n] == 0).
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace gd {

namespace {

constexpr int BLOCK = GD_LIVE_ROWS_BLOCK, LANES = 256, PER_LANE = BLOCK / LANES, WAVES = LANES / 64;

// the lane's four rows: bit j of the result is row base + j
template <bool ZERO>
__device__ __forceinline__ unsigned lane_bits(const uint8_t *__restrict__ mask, int n, int base) {
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < PER_LANE; j++)
        if (base + j < n && (mask[base + j] != 0) != ZERO) bits |= 1u << j;
    return bits;
}

__device__ __forceinline__ int wave_total(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool ZERO>
__global__ __launch_bounds__(LANES) void k_live_count(const uint8_t *__restrict__ mask, int n, int32_t *__restrict__ scratch) {
    __shared__ int s_wave[WAVES];
    const int tid = threadIdx.x;
    const int c = wave_total(__popc(lane_bits<ZERO>(mask, n, blockIdx.x * BLOCK + tid * PER_LANE)));
    if ((tid & 63) == 0) s_wave[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; v++) total += s_wave[v];
        scratch[blockIdx.x] = total;
    }
}

template <bool ZERO>
__global__ __launch_bounds__(LANES) void k_live_write(const uint8_t *__restrict__ mask, int n, const int32_t *__restrict__ scratch,
                                                      int32_t *__restrict__ rows, int32_t *__restrict__ count,
                                                      int32_t *__restrict__ count_copy) {
    __shared__ int s_before[WAVES], s_wave[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, block = blockIdx.x;
    const int base = block * BLOCK + tid * PER_LANE;
    const unsigned bits = lane_bits<ZERO>(mask, n, base);
    const int c = __popc(bits);
    int incl = c;  // the inclusive scan of c over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    int before = 0;  // the set rows of the blocks before this one
    for (int i = tid; i < block; i += LANES) before += scratch[i];
    before = wave_total(before);
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_before[wave] = before;
    __syncthreads();
    int at = incl - c, total = 0;
#pragma unroll
    for (int v = 0; v < WAVES; v++) {
        at += s_before[v] + (v < wave ? s_wave[v] : 0);
        total += s_before[v] + s_wave[v];
    }
    // at < n: it counts set rows below base + j, which are distinct indices below n
#pragma unroll
    for (int j = 0; j < PER_LANE; j++)
        if (bits & (1u << j)) rows[at++] = base + j;
    if (block == (int)gridDim.x - 1 && tid == LANES - 1) {
        *count = total;
        if (count_copy) *count_copy = total;
    }
}

}  // namespace

void launch_live_rows(hipStream_t st, const uint8_t *mask, int n, int32_t *rows, int32_t *count, int32_t *scratch,
                      int32_t *count_copy, bool zero) {
    const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK);
    if (zero) {
        hipLaunchKernelGGL(k_live_count<true>, dim3(blocks), dim3(LANES), 0, st, mask, n, scratch);
        hipLaunchKernelGGL(k_live_write<true>, dim3(blocks), dim3(LANES), 0, st, mask, n, (const int32_t *)scratch, rows, count,
                           count_copy);
    } else {
        hipLaunchKernelGGL(k_live_count<false>, dim3(blocks), dim3(LANES), 0, st, mask, n, scratch);
        hipLaunchKernelGGL(k_live_write<false>, dim3(blocks), dim3(LANES), 0, st, mask, n, (const int32_t *)scratch, rows, count,
                           count_copy);
    }
}

}  // namespace gd
