// The columns of the packed observation (what GPUDriveTorchEnv.get_obs() assembles with norm_obs = True, reference
// gpudrive/env/env_torch.py:756-896, 1172-1216; normalisation in gpudrive/datatypes/observation.py:71-90, 229-262 and
// gpudrive/datatypes/roadgraph.py:329-364; constants gpudrive/env/constants.py:6-21) from one raw row of the exported tensors.
// One definition for k_pack_obs (the second pass over the exported tensors) and for the kernels that write the packed rows
// where the raw rows are produced (kernels.hip, map_obs.hip, map_obs_linear.hip), so that the two are bit-identical by
// construction.  Divisions are true IEEE divisions like torch's CPU kernels (torch's CUDA kernels multiply by the reciprocal
// of a scalar divisor, which may differ in the last bit).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gpudrive_amd.h"

namespace gd {

constexpr float kPackAgentScale = GD_VEHICLE_SCALE;  // madrona_gpudrive.vehicleScale
constexpr float kPackTwoPi = 6.283185307179586f;     // constants.MAX_ORIENTATION_RAD = 2 * np.pi

__device__ __forceinline__ float pack_norm_min_max(float x, float lo, float hi) {  // gpudrive/utils/geometry.py:15-26
    return 2.f * ((x - lo) / (hi - lo)) - 1.f;
}

// ego, env_torch.py:756-800: column c (0..5) of the packed row from the self-observation row (8 floats)
__device__ __forceinline__ float pack_ego_col(const float *self, int c) {
    switch (c) {
        case 0: return self[0] / 100.f;
        case 1: return (self[1] * kPackAgentScale) / 30.f;
        case 2: return (self[2] * kPackAgentScale) / 15.f;
        case 3: return pack_norm_min_max(self[4], -1000.f, 1000.f);
        case 4: return pack_norm_min_max(self[5], -1000.f, 1000.f);
        default: return self[6];
    }
}

// partners, env_torch.py:828-858: column c (0..5) from the raw value of the same column of the partner row (9 floats)
__device__ __forceinline__ float pack_partner_col(float x, int c) {
    const bool nm = c == 1 || c == 2;
    const float num = nm ? x - (-1000.f) : (c >= 4 ? x * kPackAgentScale : x);
    const float den = c == 0 ? 100.f : (nm ? 1000.f - (-1000.f) : (c == 3 ? kPackTwoPi : (c == 4 ? 30.f : 15.f)));
    const float q = num / den;
    return nm ? 2.f * q - 1.f : q;
}

// road points, env_torch.py:860-896: column c (0..12; 6..12 = one-hot over 7 road point types) from the raw road row (9 floats:
// x is raw column c for c < 6, the type column otherwise)
__device__ __forceinline__ float pack_road_col(float x, int c) {
    if (c >= 6) return (int)(long long)x == c - 6 ? 1.f : 0.f;
    const bool nm = c < 2;
    const float num = nm ? x - (-1000.f) : x;
    const float den = nm ? 1000.f - (-1000.f) : (c < 5 ? 100.f : kPackTwoPi);
    const float q = num / den;
    return nm ? 2.f * q - 1.f : q;
}

// the 13 packed columns of one raw road row, o[0..13)
__device__ __forceinline__ void pack_road_row(const float *raw, float *o) {
#pragma unroll
    for (int c = 0; c < 6; c++) o[c] = pack_road_col(raw[c], c);
#pragma unroll
    for (int c = 6; c < 13; c++) o[c] = pack_road_col(raw[6], c);
}
// the 6 packed columns of one raw partner row
__device__ __forceinline__ void pack_partner_row(const float *raw, float *o) {
#pragma unroll
    for (int c = 0; c < 6; c++) o[c] = pack_partner_col(raw[c], c);
}

// A span of n floats staged at `src` (LDS) stored to `dst` (global) at any dword alignment: the conditioned learner rows
// (gd_attach_packed_rows_conditioned) have the odd pitch D + 3, so row r starts at float r (D + 3) = -r (mod 4) and its road
// block at 3 - r (mod 4).  The <= 3 floats in front of dst's first 16-byte boundary and the <= 3 behind its last one leave as
// single dwords, everything between as aligned 16-byte pieces.  LDS is read a dword at a time: the shifted 16-byte reads
// would be misaligned (ds_read_b128 off a 16-byte boundary replays).  Threads tid, tid + nt, ... share the work; every dword
// of [dst, dst + n) is written exactly once and nothing outside it, so neighbouring spans of other workgroups never race.
// (tests/test_conditioned_rows.py restates the arithmetic.)
__device__ __forceinline__ void store_span(const float *src, float *dst, int n, int tid, int nt) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int phase = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    const int head = min((4 - phase) & 3, n);  // single dwords in front of the first boundary
    const int body = (n - head) >> 2;          // whole 16-byte pieces
    const int edge = n - body * 4;             // single dwords in all: head + tail, <= 6
    const float *s = src + head;
    f4 *o = reinterpret_cast<f4 *>(dst + head);
    for (int q = tid; q < body; q += nt) {
        const f4 v = {s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
        __builtin_nontemporal_store(v, o + q);
    }
    for (int e = tid; e < edge; e += nt) {
        const int k = e < head ? e : e + body * 4;
        __builtin_nontemporal_store(src[k], dst + k);
    }
}

}  // namespace gd
