// Device rollout buffer (gd_rollout_store, gd_rollout_sort, gd_rollout_gae, gd_rollout_gather): the consumer side of the
// learner step.  The reference's Experience and compute_gae (gpudrive/integrations/puffer/ppo.py:530-666, 239-245) take the
// step's tensors to the host -- torch.where(mask)[0].cpu(), five .cpu().numpy() copies and a Python list of (env_id, step)
// per step; a Python sorted(), a serial loop over the batch and a second copy of the observations per rollout.  Here the
// experience stays on the device from the step to the minibatch:
//   k_rollout_plan    one workgroup per step scans the mask (the scan of learner.hip's k_learner_rows), gives every live row
//                     that fits its storage position, writes the entry's scalars, its row and its ordinal within the row
//                     (count[row] before the lane that owns the row increments it: no atomics), and advances ptr / step /
//                     dropped;
//   k_rollout_copy    a workgroup per row copies the observation row to its position and leaves at once where there is none;
//   k_rollout_sort    idxs[offset[row[p]] + ord[p]] = p: the order of the reference's sorted() without a sort, offset being
//                     the caller's exclusive prefix sum of count; then the counters are reset;
//   k_gae_terms       delta and coef of gae_chain.hpp through idxs, in sorted order;
//   k_gae_chain       a lane per position: a head (a position behind which the chain is cut, gae_chain.hpp) walks its run
//                     down to the next head; nothing waits on another lane, wave or workgroup;
//   k_rollout_gather  minibatches as flatten_batch lays them out: a sample's observation row in 16-byte pieces split over
//                     `parts` workgroups, the first of which writes the scalars, the action and returns = adv + value.
// Every byte of every output is stored on every call.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "gae_chain.hpp"

#ifndef GD_ROLLOUT_SPLIT
#define GD_ROLLOUT_SPLIT 1  // workgroups per gathered sample: one 256-lane pass of four pieces covers a row of 4096 floats
#endif

namespace gd {

namespace {

constexpr int PLAN_THREADS = 1024;
typedef float f4 __attribute__((ext_vector_type(4)));

enum { ST_PTR = 0, ST_STEP = 1, ST_DROPPED = 2, ST_BAD = 3 };

__global__ __launch_bounds__(PLAN_THREADS) void k_rollout_plan(gd_rollout ro, const float *__restrict__ value,
                                                               const int64_t *__restrict__ action, const float *__restrict__ logprob,
                                                               const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                               const uint8_t *__restrict__ mask) {
    __shared__ int s_scan[PLAN_THREADS];
    const int t = threadIdx.x, n = ro.num_rows;
    const int chunk = (n + PLAN_THREADS - 1) / PLAN_THREADS;
    const int b = min(t * chunk, n), e = min(b + chunk, n);
    // (read before the first barrier; the last thread writes it after the last one)
    const int base = min(max(ro.state[ST_PTR], 0), ro.batch_size), room = ro.batch_size - base;
    int c = 0;
    for (int i = b; i < e; i++) c += mask[i] != 0;
    s_scan[t] = c;
    __syncthreads();
    for (int off = 1; off < PLAN_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan
        const int v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    int r = s_scan[t] - c;  // live rows in front of this chunk
    const int aw = ro.action_width;
    for (int i = b; i < e; i++) {
        int p = -1;
        if (mask[i] != 0) {
            if (r < room) {
                p = base + r;
                ro.values[p] = value[i];
                ro.logprobs[p] = logprob[i];
                ro.rewards[p] = reward[i];
                ro.dones[p] = done[i] != 0 ? 1.f : 0.f;
                for (int k = 0; k < aw; k++) ro.actions[(size_t)p * aw + k] = action[(size_t)i * aw + k];
                const int o = ro.count[i];  // row i is this lane's alone
                ro.row[p] = i;
                ro.ord[p] = o;
                ro.count[i] = o + 1;
            }
            r++;
        }
        ro.dst[i] = p;
    }
    if (t == PLAN_THREADS - 1) {
        const int live = s_scan[t], k = min(live, room);
        ro.state[ST_PTR] = base + k;
        ro.state[ST_STEP] += 1;
        ro.state[ST_DROPPED] += live - k;
    }
}

// VEC: rows are whole 16-byte pieces at both ends (obs_width % 4 == 0 and both pointers aligned); otherwise rows start at
// every dword phase and are copied dword by dword -- a workgroup owns whole rows and a dword store shares nothing with a
// neighbour.  NT: the storage is read an epoch later and is far larger than the caches.
template <bool VEC, bool NT>
__global__ __launch_bounds__(256) void k_rollout_copy(gd_rollout ro, const float *__restrict__ obs) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const int p = ro.dst[i];
    if (p < 0 || p >= ro.batch_size) return;  // (uniform over the workgroup)
    const size_t w = (size_t)ro.obs_width;
    if constexpr (VEC) {
        const int nq = ro.obs_width >> 2;
        const f4 *src = reinterpret_cast<const f4 *>(obs + (size_t)i * w);
        f4 *dst = reinterpret_cast<f4 *>(ro.obs + (size_t)p * w);
        for (int q0 = tid; q0 < nq; q0 += 4 * 256) {
            f4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                if (q < nq) v[k] = src[q];  // the step's kernels wrote it just now: a plain load
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                if (q < nq) {
                    if constexpr (NT) __builtin_nontemporal_store(v[k], dst + q);
                    else dst[q] = v[k];
                }
            }
        }
    } else {
        const float *src = obs + (size_t)i * w;
        float *dst = ro.obs + (size_t)p * w;
        for (int q = tid; q < ro.obs_width; q += 256) {
            if constexpr (NT) __builtin_nontemporal_store(src[q], dst + q);
            else dst[q] = src[q];
        }
    }
}

__global__ __launch_bounds__(256) void k_rollout_sort(gd_rollout ro, const int64_t *__restrict__ offset, int64_t *__restrict__ idxs) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < ro.batch_size) {
        const int row = ro.row[p];
        bool ok = row >= 0 && row < ro.num_rows;
        if (ok) {
            const long long s = offset[row] + ro.ord[p];
            ok = s >= 0 && s < ro.batch_size;
            if (ok) idxs[s] = p;
        }
        if (!ok) atomicAdd(ro.state + ST_BAD, 1);
    }
    // count is not read here (offset is the caller's copy of its prefix sum): reset for the next rollout
    if (p < ro.num_rows) ro.count[p] = 0;
    if (p == 0) ro.state[ST_PTR] = 0, ro.state[ST_STEP] = 0;
}

__global__ __launch_bounds__(256) void k_gae_terms(gd_rollout ro, const int64_t *__restrict__ idxs, float gamma, float gl,
                                                   float *__restrict__ delta, float *__restrict__ coef) {
    const int t = blockIdx.x * 256 + threadIdx.x, n = ro.batch_size;
    if (t >= n) return;
    float dl = 0.f, cf = 0.f;  // position n-1 has no term; a position that cannot be read is a cut with delta 0
    if (t < n - 1) {
        const long long p0 = idxs[t], p1 = idxs[t + 1];
        if (p0 >= 0 && p0 < n && p1 >= 0 && p1 < n)
            gae_chain::terms(gamma, gl, ro.rewards[p1], ro.values[p1], ro.dones[p1], ro.values[p0], dl, cf);
        else
            atomicAdd(ro.state + ST_BAD, 1);
    }
    delta[t] = dl;
    coef[t] = cf;
}

__global__ __launch_bounds__(256) void k_gae_chain(int n, const float *__restrict__ delta, const float *__restrict__ coef,
                                                   float *__restrict__ adv) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (t == n - 1) {
        adv[t] = 0.f;
        return;
    }
    if (!gae_chain::is_head(coef[t], t, n)) return;
    gae_chain::run(t, [&](long long k, float &dl, float &cf) { dl = delta[k], cf = coef[k]; }, [&](long long k, float a) { adv[k] = a; });
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_rollout_gather(gd_rollout ro, gd_rollout_batch b, int parts) {
    const int smp = blockIdx.x / parts, part = blockIdx.x - smp * parts, tid = threadIdx.x;
    // sample smp = (m, r, h) of [n][minibatch_rows][bptt_horizon]
    const int per_mb = b.minibatch_rows * b.bptt_horizon;
    const int m = smp / per_mb, rh = smp - m * per_mb, r = rh / b.bptt_horizon, h = rh - r * b.bptt_horizon;
    const long long s = ((long long)r * b.num_minibatches + (b.first + m)) * b.bptt_horizon + h;
    const bool in = s >= 0 && s < ro.batch_size;  // (holds for every sample of a checked launch)
    const long long pp = in ? b.idxs[s] : -1;
    const bool ok = pp >= 0 && pp < ro.batch_size;
    const size_t p = ok ? (size_t)pp : 0, w = (size_t)ro.obs_width;
    if constexpr (VEC) {
        const int nq = ro.obs_width >> 2, chunk = (nq + parts - 1) / parts;
        const int lo = part * chunk, hi = min(nq, lo + chunk);
        const f4 *src = reinterpret_cast<const f4 *>(ro.obs + p * w);
        f4 *dst = reinterpret_cast<f4 *>(b.obs + (size_t)smp * w);
        for (int q0 = lo + tid; q0 < hi; q0 += 4 * 256) {
            f4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                v[k] = f4{0.f, 0.f, 0.f, 0.f};
                // the storage is far larger than the Infinity Cache and read once per epoch: non-temporal
                if (q < hi && ok) v[k] = __builtin_nontemporal_load(src + q);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q0 + k * 256;
                if (q < hi) dst[q] = v[k];  // read by the policy next: a plain store
            }
        }
    } else {
        const int nw = ro.obs_width, chunk = (nw + parts - 1) / parts;
        const int lo = part * chunk, hi = min(nw, lo + chunk);
        const float *src = ro.obs + p * w;
        float *dst = b.obs + (size_t)smp * w;
        for (int q = lo + tid; q < hi; q += 256) dst[q] = ok ? __builtin_nontemporal_load(src + q) : 0.f;
    }
    if (part != 0) return;

    const int aw = ro.action_width;
    for (int k = tid; k < aw; k += 256) b.actions[(size_t)smp * aw + k] = ok ? ro.actions[p * aw + k] : 0;
    if (tid == 0) {
        const float v = ok ? ro.values[p] : 0.f, a = in ? b.advantages[s] : 0.f;
        b.logprobs[smp] = ok ? ro.logprobs[p] : 0.f;
        b.dones[smp] = ok ? ro.dones[p] : 0.f;
        b.values[smp] = v;
        b.advantages_out[smp] = a;
        b.returns[smp] = a + v;
        if (!ok) atomicAdd(ro.state + ST_BAD, 1);
    }
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

void launch_rollout_store(const gd_rollout &ro, hipStream_t st, const float *obs, const float *value, const int64_t *action,
                          const float *logprob, const float *reward, const uint8_t *done, const uint8_t *mask, bool streaming) {
    hipLaunchKernelGGL(k_rollout_plan, dim3(1), dim3(PLAN_THREADS), 0, st, ro, value, action, logprob, reward, done, mask);
    const dim3 grid((unsigned)ro.num_rows);
    const bool vec = ro.obs_width % 4 == 0 && aligned16(obs) && aligned16(ro.obs);
    if (vec) {
        if (streaming) hipLaunchKernelGGL((k_rollout_copy<true, true>), grid, dim3(256), 0, st, ro, obs);
        else hipLaunchKernelGGL((k_rollout_copy<true, false>), grid, dim3(256), 0, st, ro, obs);
    } else {
        if (streaming) hipLaunchKernelGGL((k_rollout_copy<false, true>), grid, dim3(256), 0, st, ro, obs);
        else hipLaunchKernelGGL((k_rollout_copy<false, false>), grid, dim3(256), 0, st, ro, obs);
    }
}

void launch_rollout_sort(const gd_rollout &ro, hipStream_t st, const int64_t *offset, int64_t *idxs) {
    const int n = std::max(ro.batch_size, ro.num_rows);
    hipLaunchKernelGGL(k_rollout_sort, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ro, offset, idxs);
}

void launch_rollout_gae(const gd_rollout &ro, hipStream_t st, const int64_t *idxs, float gamma, float gae_lambda, float *delta,
                        float *coef, float *adv) {
    const dim3 grid((unsigned)((ro.batch_size + 255) / 256));
    const float gl = gamma * gae_lambda;
    hipLaunchKernelGGL(k_gae_terms, grid, dim3(256), 0, st, ro, idxs, gamma, gl, delta, coef);
    hipLaunchKernelGGL(k_gae_chain, grid, dim3(256), 0, st, ro.batch_size, delta, coef, adv);
}

void launch_rollout_gather(const gd_rollout &ro, hipStream_t st, const gd_rollout_batch &b) {
    const int parts = b.split > 0 ? b.split : GD_ROLLOUT_SPLIT;
    const long long samples = (long long)b.n * b.minibatch_rows * b.bptt_horizon;
    const dim3 grid((unsigned)(samples * parts));
    const bool vec = ro.obs_width % 4 == 0 && aligned16(ro.obs) && aligned16(b.obs);
    if (vec) hipLaunchKernelGGL(k_rollout_gather<true>, grid, dim3(256), 0, st, ro, b, parts);
    else hipLaunchKernelGGL(k_rollout_gather<false>, grid, dim3(256), 0, st, ro, b, parts);
}

}  // namespace gd
