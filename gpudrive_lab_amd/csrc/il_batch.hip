// Device expert dataset (gd_il_index, gd_il_batch, gd_il_future_batch): the consumer side of the expert trajectory recorder.  The reference's
// ExpertDataset (gpudrive/integrations/il/dataloader.py:5-71, 183-211) pads a second copy of every recorded array, lists the
// valid (row, time) pairs in Python and slices one sample at a time in DataLoader workers; baselines/il/il.py:248-263 then
// copies each collated batch to the device.  Here the recorder's arrays stay where record.hip wrote them:
//   k_il_index    a wave per source row evaluates the 91 valid flags (dataloader.py:16-23) in two 64-lane passes and ballots
//                 them: the first launch counts, the second writes the row's entries at the row's offset, ascending in time by
//                 ballot prefix (np.where order, dataloader.py:66-71);
//   k_il_batch    one launch gathers a batch: a sample's R stacked observation rows are one contiguous span of the dataset
//                 and one of the batch (16-byte pieces, zeros in front of t = 0), split over `parts` workgroups; the first of
//                 them also writes the action targets, both masks and the sample's (idx1, idx2);
//   k_il_future   (gd_il_future_batch) the same gather with the linear-probing dataset's outputs -- the reference's
//                 FutureDataset (gpudrive/integrations/il/linear_probing/dataloader.py): valid_mask and ego_mask beside the
//                 targets, and the future mask and the 64-class future position labels, computed per sample by the last
//                 of its workgroups from the ego's recorded pose and one more observation row.
// Every byte of every output is stored on every call: the padding is written, never assumed.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "gd_math.hpp"

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

// one position of sel, decoded: the entry's (shard, row, idx2, idx1), or ok = false for a position outside the index and for
// an entry that names no (row, time) of the dataset -- padding, nothing is read through it
struct il_sample {
    int s, row, idx2, idx1;
    bool ok;
};

__device__ __forceinline__ il_sample il_decode(const gd_il_dataset &ds, const int32_t *entries, long long n_entries,
                                               const int64_t *sel, int smp) {
    const long long pos = sel[smp];
    il_sample e{0, 0, 0, 0, pos >= 0 && pos < n_entries};
    if (e.ok) {
        const int4 v = reinterpret_cast<const int4 *>(entries)[pos];
        e.s = v.x, e.row = v.y, e.idx2 = v.z, e.idx1 = v.w;
        e.ok = e.s >= 0 && e.s < ds.n_shards && e.idx2 >= 0 && e.idx2 <= T - ds.pred_len;
        e.ok = e.ok && e.row >= 0 && e.row < ds.shard[e.s].n_rows;
        if (!e.ok) e.s = 0;
    }
    return e;
}

// A span of n flag bytes at an odd pitch.  Neighbouring samples share dwords, so the calling workgroup, the span's one
// owner, stores the bytes in front of the first 4-byte boundary and behind the last one singly and whole dwords between
// (pack_cols.hpp's store_span, on bytes)
template <class F>
__device__ __forceinline__ void il_store_flags(uint8_t *dst, int n, int tid, F flag) {
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

// obs: this workgroup's share, pieces [lo, hi) of the sample's R * Q
template <int A_T>
__device__ __forceinline__ void il_copy_obs(const gd_il_dataset &ds, const gd_il_shard &sh, const il_sample &e, float *obs,
                                            int smp, int part, int parts, int tid) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13, Q = D / 4;
    static_assert(D % 4 == 0, "observation rows are whole 16-byte pieces");
    const int R = ds.rollout_len;
    const int t0 = e.idx2 - R + 1, z = e.ok ? max(0, -t0) : R;
    const int nq = R * Q, chunk = (nq + parts - 1) / parts;
    const int lo = part * chunk, hi = min(nq, lo + chunk), zq = z * Q;
    const f4 *src = reinterpret_cast<const f4 *>(sh.obs) + (long long)e.row * T * Q;
    const long long off = (long long)t0 * Q;  // (negative only where q < zq)
    f4 *dst = reinterpret_cast<f4 *>(obs) + (long long)smp * nq;
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

// the action targets and both window masks of one sample: the work of the sample's first workgroup
template <int A_T>
__device__ __forceinline__ void il_copy_targets(const gd_il_dataset &ds, const gd_il_shard &sh, const il_sample &e, float *actions,
                                                uint8_t *road_mask, uint8_t *partner_mask, int smp, int tid) {
    constexpr int PM = A_T - 1, RW = K / 8;
    static_assert(K % 8 == 0, "road mask rows are whole 8-byte words");
    const int R = ds.rollout_len, P = ds.pred_len;
    // (the window's geometry is three integers worked out again here and not carried in il_sample: carried, they cost
    // k_il_batch two more SGPRs)
    const int t0 = e.idx2 - R + 1;             // the time of the sample's first stacked row
    const int z = e.ok ? max(0, -t0) : R;      // stacked rows in front of t = 0: padding
    const long long first = (long long)e.row * T;  // (row, 0) in units of one time step
    {  // actions: P * 3 floats from (row, idx2) on
        const float *src = sh.actions + (first + e.idx2) * 3;
        float *dst = actions + (long long)smp * P * 3;
        for (int i = tid; i < P * 3; i += 256) dst[i] = e.ok ? src[i] : 0.f;
    }
    {  // road_mask: rows of 200 bytes, 8-byte aligned at both ends
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(sh.road_mask) + first * RW;
        const long long off = (long long)t0 * RW;
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(road_mask) + (long long)smp * R * RW;
        const int zw = z * RW;
        for (int w = tid; w < R * RW; w += 256) dst[w] = w >= zw ? src[w + off] : 0x0101010101010101ull;
    }
    {  // partner_mask: a span of R * (A - 1) bytes at an odd pitch
        const uint8_t *src = sh.partner_mask + first * PM;
        const long long off = (long long)t0 * PM;
        const int n = R * PM, zb = z * PM;
        il_store_flags(partner_mask + (long long)smp * n, n, tid,
                       [&](int i) -> uint32_t { return i >= zb ? (src[i + off] == 2 ? 1u : 0u) : 1u; });
    }
}

template <int A_T>
__global__ __launch_bounds__(256) void k_il_batch(gd_il_dataset ds, gd_il_batch_buffers b, int parts) {
    const int smp = blockIdx.x / parts, part = blockIdx.x - smp * parts, tid = threadIdx.x;
    const il_sample e = il_decode(ds, b.entries, b.n_entries, b.sel, smp);
    const gd_il_shard &sh = ds.shard[e.s];
    il_copy_obs<A_T>(ds, sh, e, b.obs, smp, part, parts, tid);
    if (part != 0) return;

    if (tid == 0) {
        b.data_idx[2 * (long long)smp + 0] = e.ok ? e.idx1 : -1;
        b.data_idx[2 * (long long)smp + 1] = e.ok ? e.idx2 : -1;
        if (!e.ok) atomicAdd(b.bad_indices, 1);
    }
    il_copy_targets<A_T>(ds, sh, e, b.actions, b.road_mask, b.partner_mask, smp, tid);
}

// numpy.digitize(v, edges) - 1 clipped to [0, 7]: an edge counts unless it is greater than v, so that a NaN counts all nine
__device__ __forceinline__ int il_class(float v, const double (&edges)[9]) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) n += !(edges[i] > (double)v);
    return min(max(n - 1, 0), 7);
}

// constants.py's normalisation of a relative position, (MIN, MAX) = (-1000, 1000), as dataloader.py:110 spells it
__device__ __forceinline__ float il_norm(float v) { return 2.f * ((v - (-1000.f)) / 2000.f) - 1.f; }

// k_il_batch with the linear-probing outputs (gd_il_future_batch).  The window is copied by the same code; the first of a
// sample's workgroups adds valid_mask and ego_mask to the targets, the LAST one computes the future mask and labels (with one
// workgroup per sample the two coincide).  The sines and cosines are uniform over a sample: lane 0 evaluates them.
template <int A_T, int EXP>
__global__ __launch_bounds__(256) void k_il_future(gd_il_dataset ds, gd_il_future fu, gd_il_future_buffers b, int parts) {
    constexpr int PM = A_T - 1, NB = (6 + PM * 6) / 4;  // 16-byte pieces of the ego and partner blocks of one observation row
    static_assert((6 + PM * 6) % 4 == 0, "the partner block ends on a 16-byte boundary");
    const int R = ds.rollout_len, P = ds.pred_len, F = fu.future_step;
    const int smp = blockIdx.x / parts, part = blockIdx.x - smp * parts, tid = threadIdx.x;
    const il_sample e = il_decode(ds, b.entries, b.n_entries, b.sel, smp);
    const gd_il_shard &sh = ds.shard[e.s];
    il_copy_obs<A_T>(ds, sh, e, b.obs, smp, part, parts, tid);

    if (part == 0) {
        if (tid == 0) {
            b.valid_mask[smp] = e.ok && il_valid(sh, e.row, e.idx2 + P - 1);
            if (!e.ok) atomicAdd(b.bad_indices, 1);
        }
        // ego_mask: R bytes at any pitch, stored singly
        for (int r = tid; r < R; r += 256) {
            const int t = e.idx2 - R + 1 + r;
            b.ego_mask[(long long)smp * R + r] = e.ok && t >= 0 && il_valid(sh, e.row, t);
        }
        il_copy_targets<A_T>(ds, sh, e, b.actions, b.road_mask, b.partner_mask, smp, tid);
    }
    if (part != parts - 1) return;

    const int tf = e.idx2 + F;                 // the future time
    const bool ahead = e.ok && tf < T;         // ... lies inside the episode
    const long long now = (long long)e.row * T + e.idx2;
    const int padding = il_class(0.f, fu.xbins) * 8 + il_class(0.f, fu.ybins);  // the label of the raw pair (0, 0)
    if constexpr (EXP == GD_IL_FUTURE_EGO) {
        if (tid != 0) return;
        int label = padding;
        if (ahead) {
            const float *pos = fu.ego_global_pos[e.s] + now * 2;
            float s, c;
            p_sincos(fu.ego_global_rot[e.s][now], s, c);
            const float dx = pos[2 * F] - pos[0], dy = pos[2 * F + 1] - pos[1];
            const float rx = dx * c + dy * s, ry = (-dx) * s + dy * c;
            label = il_class(il_norm(rx), fu.xbins) * 8 + il_class(il_norm(ry), fu.ybins);
        }
        b.future_mask[smp] = ahead && il_valid(sh, e.row, e.idx2) && il_valid(sh, e.row, tf);
        b.future_pos[smp] = label;
    } else {
        __shared__ f4 block[NB];       // columns [0, 6 + (A - 1) * 6) of the observation row at the future time
        __shared__ float rot[4];       // cos, sin of rot[tf]; cos, sin of -rot[idx2]
        __shared__ uint8_t flags[A_T];
        if (ahead) {
            // whole 16-byte pieces, coalesced; read once, like the window
            const f4 *src = reinterpret_cast<const f4 *>(sh.obs) + (now + F) * ((6 + PM * 6 + K * 13) / 4);
            for (int q = tid; q < NB; q += 256) block[q] = __builtin_nontemporal_load(src + q);
            if (tid == 0) {
                p_sincos(fu.ego_global_rot[e.s][now + F], rot[1], rot[0]);
                p_sincos(-fu.ego_global_rot[e.s][now], rot[3], rot[2]);
            }
        }
        __syncthreads();
        if (tid < PM) {
            const int j = tid;
            bool aux = true;
            int label = padding;
            if (ahead) aux = sh.partner_mask[now * PM + j] != 0 || sh.partner_mask[(now + F) * PM + j] != 0;
            if (!aux) {
                const float *col = reinterpret_cast<const float *>(block) + 6 + 6 * j;
                const float px = col[1] * 1000.f, py = col[2] * 1000.f;
                const float *pos = fu.ego_global_pos[e.s] + now * 2;
                const float c = rot[0], s = rot[1], c2 = rot[2], s2 = rot[3];
                const float gx = (pos[2 * F] + px * c) - py * s, gy = (pos[2 * F + 1] + px * s) + py * c;
                const float dx = gx - pos[0], dy = gy - pos[1];
                const float cx = dx * c2 + dy * s2, cy = (-dx) * s2 + dy * c2;
                label = il_class(il_norm(cx), fu.xbins) * 8 + il_class(il_norm(cy), fu.ybins);
            }
            b.future_pos[(long long)smp * PM + j] = label;  // rows of (A - 1) * 8 bytes: 8-byte aligned at any A
            flags[j] = aux;
        }
        __syncthreads();
        il_store_flags(b.future_mask + (long long)smp * PM, PM, tid, [&](int i) -> uint32_t { return flags[i]; });
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

void launch_il_future(const gd_il_dataset &ds, const gd_il_future &fu, hipStream_t st, const gd_il_future_buffers &b, int split) {
    if (b.batch == 0) return;
    const int parts = split > 0 ? split : GD_IL_SPLIT;
    const dim3 grid((unsigned)b.batch * (unsigned)parts);
    const bool ego = fu.exp == GD_IL_FUTURE_EGO;
    if (ds.max_agents == 64) {
        if (ego) hipLaunchKernelGGL((k_il_future<64, GD_IL_FUTURE_EGO>), grid, dim3(256), 0, st, ds, fu, b, parts);
        else hipLaunchKernelGGL((k_il_future<64, GD_IL_FUTURE_OTHER>), grid, dim3(256), 0, st, ds, fu, b, parts);
    } else {
        if (ego) hipLaunchKernelGGL((k_il_future<128, GD_IL_FUTURE_EGO>), grid, dim3(256), 0, st, ds, fu, b, parts);
        else hipLaunchKernelGGL((k_il_future<128, GD_IL_FUTURE_OTHER>), grid, dim3(256), 0, st, ds, fu, b, parts);
    }
}

}  // namespace gd
