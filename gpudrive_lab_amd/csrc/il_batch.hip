// Device expert dataset (gd_il_index, gd_il_batch): the consumer side of the expert trajectory recorder.  The reference's
// ExpertDataset (gpudrive/integrations/il/dataloader.py:5-71, 183-211) pads a second copy of every recorded array, lists the
// valid (row, time) pairs in Python and slices one sample at a time in DataLoader workers; baselines/il/il.py:248-263 then
// copies each collated batch to the device.  Here the recorder's arrays stay where record.hip wrote them:
//   k_il_index    a wave per source row evaluates the 91 valid flags (dataloader.py:16-23) in two 64-lane passes and ballots
//                 them: the first launch counts, the second writes the row's entries at the row's offset, ascending in time by
//                 ballot prefix (np.where order, dataloader.py:66-71);
//   k_il_batch    one launch gathers a batch: a sample's R stacked observation rows are one contiguous span of the dataset
//                 and one of the batch (16-byte pieces, zeros in front of t = 0), split over `parts` workgroups; the first of
//                 them also writes the action targets, both masks and the sample's (idx1, idx2).
// Every byte of every output is stored on every call: the padding is written, never assumed.
#include <hip/hip_runtime.h>

#include "engine.hpp"

#ifndef GD_IL_SPLIT
#define GD_IL_SPLIT 4  // workgroups per sample (NOTEBOOK.md, "Device expert dataset": 1, 2 and 4 measure alike at B = 512)
#endif

namespace gd {

namespace {

constexpr int K = GD_MAP_OBS_K;
constexpr int T = GD_EPISODE_LEN;
typedef float f4 __attribute__((ext_vector_type(4)));

// dataloader.py:16-18 on one (row, time): strict compares in fp32, so a NaN component leaves the step valid
__device__ __forceinline__ bool il_valid(const gd_il_shard &sh, int row, int t) {
    const size_t nt = (size_t)row * T + t;
    const float *a = sh.actions + nt * 3;
    return sh.dead_mask[nt] == 0 && !(fabsf(a[1]) > 0.5f || fabsf(a[0]) > 5.f || fabsf(a[2]) > 0.2f);
}

// source row g of the shards in order -> (shard, local row); false past the last row
__device__ __forceinline__ bool il_locate(const gd_il_dataset &ds, int g, int &s, int &row) {
    for (s = 0; s < ds.n_shards; s++) {
        if (g < ds.shard[s].n_rows) {
            row = g;
            return true;
        }
        g -= ds.shard[s].n_rows;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_il_index(gd_il_dataset ds, int32_t *counts, int32_t *kept, const int64_t *entry_offset,
                                                  const int64_t *kept_ordinal, int32_t *entries) {
    const int g = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    int s, row;
    if (!il_locate(ds, g, s, row)) return;  // (uniform over the wave)
    const gd_il_shard &sh = ds.shard[s];
    const bool keep = sh.keep[row] != 0;
    const int last = T - ds.pred_len;  // the largest idx2
    int4 *out = nullptr;
    int idx1 = 0;
    if (entries) {
        out = reinterpret_cast<int4 *>(entries) + entry_offset[g];
        idx1 = (int)kept_ordinal[g];
    }
    int n = 0;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const int idx2 = pass * 64 + lane;
        const bool v = keep && idx2 <= last && il_valid(sh, row, idx2 + ds.pred_len - 1);
        const unsigned long long m = __ballot(v);
        if (out && v) out[n + __popcll(m & ((1ull << lane) - 1ull))] = make_int4(s, row, idx2, idx1);
        n += __popcll(m);
    }
    if (!entries && lane == 0) {
        counts[g] = n;
        kept[g] = keep ? 1 : 0;
    }
}

template <int A_T>
__global__ __launch_bounds__(256) void k_il_batch(gd_il_dataset ds, gd_il_batch_buffers b, int parts) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13, Q = D / 4, PM = A_T - 1, RW = K / 8;
    static_assert(D % 4 == 0 && K % 8 == 0, "observation rows are whole 16-byte pieces, road mask rows whole 8-byte words");
    const int R = ds.rollout_len, P = ds.pred_len;
    const int smp = blockIdx.x / parts, part = blockIdx.x - smp * parts, tid = threadIdx.x;

    const long long pos = b.sel[smp];
    int s = 0, row = 0, idx2 = 0, idx1 = 0;
    bool ok = pos >= 0 && pos < b.n_entries;
    if (ok) {
        const int4 e = reinterpret_cast<const int4 *>(b.entries)[pos];
        s = e.x, row = e.y, idx2 = e.z, idx1 = e.w;
        // an entry that names no (row, time) of the dataset is padding too: nothing is read through it
        ok = s >= 0 && s < ds.n_shards && idx2 >= 0 && idx2 <= T - P;
        ok = ok && row >= 0 && row < ds.shard[s].n_rows;
        if (!ok) s = 0;
    }
    const gd_il_shard &sh = ds.shard[s];
    const int t0 = idx2 - R + 1;              // the time of the sample's first stacked row
    const int z = ok ? max(0, -t0) : R;       // stacked rows in front of t = 0: padding
    const long long first = (long long)row * T;  // (row, 0) in units of one time step

    {  // obs: pieces [lo, hi) of the sample's R * Q
        const int nq = R * Q, chunk = (nq + parts - 1) / parts;
        const int lo = part * chunk, hi = min(nq, lo + chunk), zq = z * Q;
        const f4 *src = reinterpret_cast<const f4 *>(sh.obs) + first * Q;
        const long long off = (long long)t0 * Q;  // (negative only where q < zq)
        f4 *dst = reinterpret_cast<f4 *>(b.obs) + (long long)smp * nq;
        for (int q0 = lo + tid; q0 < hi; q0 += 4 * 256) {
            f4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                v[k] = f4{0.f, 0.f, 0.f, 0.f};
                // the dataset is far larger than the Infinity Cache and read once per epoch: non-temporal
                if (q < hi && q >= zq) v[k] = __builtin_nontemporal_load(src + (q + off));
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                if (q < hi) dst[q] = v[k];  // read by the model next: a plain store
            }
        }
    }
    if (part != 0) return;

    if (tid == 0) {
        b.data_idx[2 * (long long)smp + 0] = ok ? idx1 : -1;
        b.data_idx[2 * (long long)smp + 1] = ok ? idx2 : -1;
        if (!ok) atomicAdd(b.bad_indices, 1);
    }
    {  // actions: P * 3 floats from (row, idx2) on
        const float *src = sh.actions + (first + idx2) * 3;
        float *dst = b.actions + (long long)smp * P * 3;
        for (int i = tid; i < P * 3; i += 256) dst[i] = ok ? src[i] : 0.f;
    }
    {  // road_mask: rows of 200 bytes, 8-byte aligned at both ends
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(sh.road_mask) + first * RW;
        const long long off = (long long)t0 * RW;
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(b.road_mask) + (long long)smp * R * RW;
        const int zw = z * RW;
        for (int w = tid; w < R * RW; w += 256) dst[w] = w >= zw ? src[w + off] : 0x0101010101010101ull;
    }
    {  // partner_mask: a span of R * (A - 1) bytes at an odd pitch.  Neighbouring samples share dwords, so this workgroup, the
       // span's one owner, stores the bytes in front of the first 4-byte boundary and behind the last one singly and whole
       // dwords between (pack_cols.hpp's store_span, on bytes)
        const uint8_t *src = sh.partner_mask + first * PM;
        const long long off = (long long)t0 * PM;
        const int n = R * PM, zb = z * PM;
        uint8_t *dst = b.partner_mask + (long long)smp * n;
        auto flag = [&](int i) -> uint32_t { return i >= zb ? (src[i + off] == 2 ? 1u : 0u) : 1u; };
        const int head = min((int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), n);
        const int body = (n - head) >> 2;     // whole dwords
        const int edge = n - body * 4;        // single bytes in all: head + tail, <= 6
        for (int k = tid; k < body; k += 256) {
            const int i = head + 4 * k;
            *reinterpret_cast<uint32_t *>(dst + i) = flag(i) | flag(i + 1) << 8 | flag(i + 2) << 16 | flag(i + 3) << 24;
        }
        for (int e = tid; e < edge; e += 256) {
            const int i = e < head ? e : e + body * 4;
            dst[i] = (uint8_t)flag(i);
        }
    }
}

}  // namespace

void launch_il_index(const gd_il_dataset &ds, hipStream_t st, int64_t rows, int32_t *counts, int32_t *kept,
                     const int64_t *entry_offset, const int64_t *kept_ordinal, int32_t *entries) {
    if (rows == 0) return;
    hipLaunchKernelGGL(k_il_index, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, ds, counts, kept, entry_offset, kept_ordinal,
                       entries);
}

void launch_il_batch(const gd_il_dataset &ds, hipStream_t st, const gd_il_batch_buffers &b, int split) {
    if (b.batch == 0) return;
    const int parts = split > 0 ? split : GD_IL_SPLIT;
    const dim3 grid((unsigned)b.batch * (unsigned)parts);
    if (ds.max_agents == 64) hipLaunchKernelGGL(k_il_batch<64>, grid, dim3(256), 0, st, ds, b, parts);
    else hipLaunchKernelGGL(k_il_batch<128>, grid, dim3(256), 0, st, ds, b, parts);
}

}  // namespace gd
