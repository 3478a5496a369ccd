// gd_owned_rows: a byte mask [n] and an owner byte [n] to ONE segmented row list, a segment per policy, on the device.
// Segment p holds the rows with mask != 0 && owner == p in ascending order and starts at a multiple of 32
// (multi_policy_rule.hpp: segment_starts); the positions between a segment's end and the next start hold -1.
// gd_live_rows' two launches over blocks of GD_LIVE_ROWS_BLOCK = 1024 rows (256 lanes, four consecutive rows to a lane), once
// per owner inside each kernel:
//   k_owned_count   scratch[p * blocks + block] = the block's rows of owner p with a set byte
//   k_owned_write   every block adds up, per owner, scratch[p][0 .. block) for its first position in the segment and
//                   scratch[p][0 .. blocks) for the segment's length, derives the starts, scans its own 1024 rows per owner (a
//                   lane's four, a shuffle scan over the wave, the four waves through LDS) and stores its indices in order; the
//                   last block also stores the padding, count[P], start[P + 1] and, when the caller keeps a record, the counts
//                   again to count_copy[P]
// No atomics: a position is a sum of integers, so equal input gives equal bytes.  rows[start[P] ..) is not written; a row
// whose owner is >= P is listed nowhere.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "multi_policy_rule.hpp"

namespace gd {

namespace {

namespace MP = multi_policy_rule;

constexpr int BLOCK = GD_LIVE_ROWS_BLOCK, LANES = 256, PER_LANE = BLOCK / LANES, WAVES = LANES / 64;
constexpr int MAXP = GD_POLICY_SET_MAX;
static_assert(MAXP == MP::MAX_POLICIES, "the rule header and the C header disagree");

// the lane's four rows: byte j of the result is 1 + owner of row base + j when the row's mask byte is set, 0 otherwise
__device__ __forceinline__ unsigned lane_owners(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ owner, int n, int base) {
    unsigned tags = 0;
#pragma unroll
    for (int j = 0; j < PER_LANE; j++)
        if (base + j < n && mask[base + j] != 0) {
            const unsigned o = owner[base + j];
            if (o < (unsigned)MAXP) tags |= (o + 1u) << (8 * j);
        }
    return tags;
}

// bit j: row base + j is a set row of owner p
__device__ __forceinline__ unsigned owner_bits(unsigned tags, int p) {
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < PER_LANE; j++)
        if (((tags >> (8 * j)) & 0xFFu) == (unsigned)(p + 1)) bits |= 1u << j;
    return bits;
}

__device__ __forceinline__ int wave_total(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(LANES) void k_owned_count(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ owner, int n,
                                                       int P, int32_t *__restrict__ scratch) {
    __shared__ int s_wave[MAXP][WAVES];
    const int tid = threadIdx.x;
    const unsigned tags = lane_owners(mask, owner, n, blockIdx.x * BLOCK + tid * PER_LANE);
#pragma unroll
    for (int p = 0; p < MAXP; p++)
        if (p < P) {
            const int c = wave_total(__popc(owner_bits(tags, p)));
            if ((tid & 63) == 0) s_wave[p][tid >> 6] = c;
        }
    __syncthreads();
    if (tid < P) {
        int total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; v++) total += s_wave[tid][v];
        scratch[tid * (int)gridDim.x + blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(LANES) void k_owned_write(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ owner, int n,
                                                       int P, const int32_t *__restrict__ scratch, int32_t *__restrict__ rows,
                                                       int32_t *__restrict__ start, int32_t *__restrict__ count,
                                                       int32_t *__restrict__ count_copy) {
    __shared__ int s_before[MAXP][WAVES], s_total[MAXP][WAVES], s_wave[MAXP][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, block = blockIdx.x, blocks = gridDim.x;
    const int base = block * BLOCK + tid * PER_LANE;
    const unsigned tags = lane_owners(mask, owner, n, base);
    int excl[MAXP];  // the lane's set rows of owner p come after this many of its wave's (static indices: registers)
#pragma unroll
    for (int p = 0; p < MAXP; p++) {
        excl[p] = 0;
        if (p < P) {
            const int c = __popc(owner_bits(tags, p));
            int incl = c;  // the inclusive scan of c over the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(incl, d);
                if (lane >= d) incl += v;
            }
            excl[p] = incl - c;
            int before = 0, total = 0;  // owner p's set rows in the blocks before this one, and in all blocks
            for (int i = tid; i < blocks; i += LANES) {
                const int v = scratch[p * blocks + i];
                total += v;
                if (i < block) before += v;
            }
            before = wave_total(before);
            total = wave_total(total);
            if (lane == 63) s_wave[p][wave] = incl;
            if (lane == 0) s_before[p][wave] = before, s_total[p][wave] = total;
        }
    }
    __syncthreads();
    int32_t cnt[MAXP], st[MAXP + 1];
#pragma unroll
    for (int p = 0; p < MAXP; p++) {
        cnt[p] = 0;
        if (p < P)
#pragma unroll
            for (int v = 0; v < WAVES; v++) cnt[p] += s_total[p][v];
    }
    MP::segment_starts(MAXP, cnt, st);  // (count 0 past P: the starts past P repeat start[P])
    const bool last = block == blocks - 1;
#pragma unroll
    for (int p = 0; p < MAXP; p++)
        if (p < P) {
            // at < start[p] + count[p] <= n + 31 p: it counts set rows of owner p below base + j
            int at = st[p] + excl[p];
#pragma unroll
            for (int v = 0; v < WAVES; v++) at += s_before[p][v] + (v < wave ? s_wave[p][v] : 0);
            const unsigned bits = owner_bits(tags, p);
#pragma unroll
            for (int j = 0; j < PER_LANE; j++)
                if (bits & (1u << j)) rows[at++] = base + j;
            if (last) {
                const int end = st[p] + cnt[p];
                if (end + tid < st[p + 1]) rows[end + tid] = -1;  // fewer than 32 positions of padding
                if (tid == LANES - 1) {
                    start[p] = st[p];
                    start[p + 1] = st[p + 1];
                    count[p] = cnt[p];
                    if (count_copy) count_copy[p] = cnt[p];
                }
            }
        }
}

}  // namespace

void launch_owned_rows(hipStream_t st, const uint8_t *mask, const uint8_t *owner, int n, int n_policies, int32_t *rows,
                       int32_t *start, int32_t *count, int32_t *scratch, int32_t *count_copy) {
    const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_owned_count, dim3(blocks), dim3(LANES), 0, st, mask, owner, n, n_policies, scratch);
    hipLaunchKernelGGL(k_owned_write, dim3(blocks), dim3(LANES), 0, st, mask, owner, n, n_policies, (const int32_t *)scratch, rows,
                       start, count, count_copy);
}

}  // namespace gd
