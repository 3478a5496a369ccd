// The SET-UP of the rank path's selection (map_obs_rank.hip), one lane per agent and one call per 64 agent slots of a world:
// which agents take the rank path, and the checkpoints that bound each one's candidates -- first road and threshold of the
// cheap form |p - e|^2 < bound * margin (the margin covers rounding and the squared norm of the stored quaternion, like
// k_map_obs's scan) -- from its previous selection, a neighbour's, or made afresh.  What it hands to k_knn_rank, which finds the
// candidates itself (rank_cand.hpp), is a 16-byte record per agent (rk_rec) and, only for an agent that borrows a neighbour's
// checkpoints or is bounded afresh, the row of checkpoints (rk_cpf / rk_cpt, 240 B).  An agent bounded by its own checkpoints --
// every agent of an ordinary step -- has its row made by the wave that ranks it, from the checkpoints where they lie.
//
// Two callers: k_world_step (kernels.hip, the FOLD instantiations), which holds the step's final pose and runs the set-up
// itself, so that the rank path starts with k_knn_rank; and the thin kernel k_knn_scan (map_obs_rank.hip:
// GPUDRIVE_RANK_SCAN_KERNEL=1, the set-up as a launch of its own as it was, for A/B runs).  Both run the text below.
//
// The per-lane decision (`decide`) is plain C++ that a host program compiles too (tests/rank_setup_fn_model.cpp runs it
// against the expressions of the former kernel, restated there).  Every function here switches FMA contraction off for
// itself: the bits do not depend on the flags of the file that includes it.
#pragma once

#include "rank_cand.hpp"

namespace gd {
namespace rank_setup {

constexpr int RK_FAR = 1 << 30;  // rk_n: no road of the world can be within the agent's radius

// what becomes of a lane's agent
enum {
    FAR = 0,       // too far from every road of the world: the empty hand-over, no ranking
    FALLBACK = 1,  // not eligible (a small world) or bypassing: k_map_obs selects for its group
    AFRESH = 2,    // no usable bound: the workgroup's waves bound it afresh
    OWN = 3,       // bounded by its own checkpoints where they lie: the record alone
    ROW = 4        // a donor's checkpoints, or every row (GPUDRIVE_RANK_SCAN_ROWS): copied into the agent's row
};

struct Decision {
    int kind;
    int state, reason;  // rk_n, rk_ticket
    int set, n_cp;      // the checkpoint set (0: the previous selection's, 1: the episode's first) and its entries
    int donor;          // the lane whose checkpoints bound the agent, -1: its own
    float move, margin;
};

// H4: four floats x, y, z, w (float4 on the device).  h0 / h1: the agent's checkpoint headers of the two sets; hdrs: the set-0
// headers of the 64 lanes of the call (a dead lane's: zero checkpoints); bb: the world's road bounding box.
template <typename H4>
GD_RC_FN Decision decide(int self, float ex, float ey, float iw, float iz, const H4 &h0, const H4 &h1, const H4 &bb, const H4 *hdrs,
                         int R, int K, float radius, int min_roads, int max_roads, int streak, int selections, int grp,
                         bool scan_rows) {
#pragma clang fp contract(off)
    Decision o;
    o.kind = FAR; o.state = 1; o.reason = -1; o.set = 0; o.n_cp = 0; o.donor = -1; o.move = 0.f; o.margin = 0.f;
    // too far from every road of the world for any to be within the radius: no rows (a finished agent parked
    // at the padding position, src/sim.cpp:333-343)
    const float ddx = fmaxf(fmaxf(bb.x - ex, ex - bb.z), 0.f), ddy = fmaxf(fmaxf(bb.y - ey, ey - bb.w), 0.f);
    const float far = radius * 1.01f + 1.f;
    if (R >= K && ddx * ddx + ddy * ddy > far * far) {
        o.state = RK_FAR;
        return o;
    }
    // the previous selection's checkpoints, or those of the episode's first selection (a reset puts the agent
    // back where that one was made): whichever was recorded closer to where the agent is now
    const int n0 = (int)rank_cand::f32_bits(h0.z), n1 = (int)rank_cand::f32_bits(h1.z);
    const float m0 = n0 > 0 ? sqrtf((ex - h0.x) * (ex - h0.x) + (ey - h0.y) * (ey - h0.y)) : __builtin_inff();
    const float m1 = n1 > 0 ? sqrtf((ex - h1.x) * (ex - h1.x) + (ey - h1.y) * (ey - h1.y)) : __builtin_inff();
    int set = m1 < m0 ? 1 : 0;
    float move = set ? m1 : m0;
    int n_cp = set ? n1 : n0;
    // An agent far from where its own checkpoints were recorded (a logged agent back from the padding position,
    // src/sim.cpp:370-382: none at all, or the episode's first ones from somewhere else) borrows those of the
    // agent of its world whose previous selection was made nearest to where it is now: the K-th distance over a
    // prefix of the roads is a function of the position alone, 1-Lipschitz in it, whoever recorded it.  Without
    // that every road of the world was a candidate for such an agent: beyond the buffers in a world of 10,000
    // roads (the whole group of 32 to the fallback, a 3 ms step), the longest replay of the launch in smaller ones.
    if (move > rank_cand::CP_MOVE_MAX) {
        float best = move;
        int donor = -1;
        for (int j = 0; j < 64; j++) {
            const H4 hj = hdrs[j];
            const float dj = (int)rank_cand::f32_bits(hj.z) > 0 ? sqrtf((ex - hj.x) * (ex - hj.x) + (ey - hj.y) * (ey - hj.y)) : __builtin_inff();
            if (dj < best) { best = dj; donor = j; }
        }
        if (donor >= 0) {
            move = best;
            set = 0;
            n_cp = (int)rank_cand::f32_bits(hdrs[donor].z);
            o.donor = donor;
        }
    }
    const bool eligible = R >= K && R >= min_roads && R <= max_roads;  // small worlds: k_map_obs is as fast
    // a group that needed the fallback three selections in a row (agents that overflow even the long list)
    // stops paying for rank kernels whose work is thrown away; it tries again every 64th selection
    const bool bypass = eligible && streak >= 3 && ((selections + grp) & 63) != 0;
    const float z2 = iz * iz;
    const float det = (1.f - 2.f * z2) * (1.f - 2.f * z2) + 4.f * z2 * (iw * iw);
    o.margin = 1.00001f / fminf(det, 1.f);
    o.move = move; o.set = set; o.n_cp = n_cp;
    if (!eligible || bypass) {
        o.kind = FALLBACK;
        o.state = 0;
        o.reason = bypass ? -5 : -2;  // -2: a world below rk_min_roads (or without K roads)
    } else if (n_cp <= 0 || move > rank_cand::CP_MOVE_MAX) {
        // No usable bound -- the first selection after the worlds were built, a logged agent that reappears
        // anywhere on the map (src/sim.cpp:370-382) with nobody near: bounded afresh
        o.kind = AFRESH;
    } else if ((o.donor < 0 || o.donor == self) && !scan_rows) {
        // the common case: bounded by its own checkpoints (of the previous selection or the episode's first), which
        // nobody but the wave that ranks this agent writes during the ranking launch, and that one only after it
        // has read them (rank_fetch).  The row is a function of those two arrays, `move` and `margin`: lane q of
        // the ranking wave makes entry q (rank_cand.hpp cp_threshold, the running maximum as a wave scan)
        o.kind = OWN;
    } else {
        o.kind = ROW;
    }
    return o;
}
// the third word of an OWN agent's record (rk_rec: move, margin, this, -)
GD_RC_FN int own_record_bits(const Decision &o) { return o.n_cp | o.set << 8; }

}  // namespace rank_setup
}  // namespace gd

#if defined(__HIPCC__)
#include "engine.hpp"

namespace gd {
namespace rank_setup {

constexpr int K = GD_MAP_OBS_K;
constexpr int NCP = GD_RANK_NCP;

// The set-up of 64 agent slots ("a half": slots a0 .. a0 + 63 of a world) comes in three parts:
//   decide   one wave, lane l for agent a0 + l, no workgroup barrier: the decision per agent, the records, flags and empty
//            hand-overs.  No load is asked for in here and nothing is waited for.
//   rows     the whole workgroup, and only where an agent of the half borrows a neighbour's checkpoints or is bounded afresh
//            (workgroup-uniform: rows_needed): the rows of checkpoints, through the big LDS arrays.
//   list     the wave of `decide` again: the agents' places in their XCD's list (one atomicAdd per half, whose answer the wave
//            waits for: a thousand workgroups ask eight counters) and the agents into the list.
// k_world_step runs `decide` as soon as the step's pose is final, on headers it asked for with its first loads; `rows` follows
// where its phase buffer is free, in front of the partner rows, and `list` is the last thing the kernel does: every workgroup
// barrier waits for the memory operations its waves have in flight, so a wave must not carry the atomic across one.

// LDS of a half that lives from `decide` to `rows`
struct Half {
    float4 hdr[64];                  // where and how many checkpoints lane l's previous selection recorded
    int ncp[64];                     // checkpoints of lane l's row; 0: the agent is not on the rank path, or needs no row: it is
                                     // bounded by its own checkpoints, which its ranking wave reads where they are; -1: to be bounded afresh
    float p0[64], p1[64], p2[64];    // what `rows` needs of lane l's agent -- bounded afresh: position and margin; a copied row:
                                     // `move`, (source lane | set << 8) as bits, margin
    unsigned int needy[2];           // the agents to be bounded afresh (bit per lane), as `decide` saw them
    unsigned int copied[2];          // the agents whose row is copied (a donor's, GPUDRIVE_RANK_SCAN_ROWS)
};
// LDS of `rows` alone (any 16-byte aligned LDS that nobody else uses during the call)
struct Rows {
    unsigned int hist[4][256];       // per wave: histogram of squared distances of the roads streamed so far
    float thr[NCP][64];              // checkpoint q of lane l: the threshold it gives ...
    unsigned short first[NCP][64];   // ... and the first road it holds for (running maximum: rank_cand.hpp)
};
static_assert(sizeof(Half) % 16 == 0 && sizeof(Rows) % 16 == 0, "callers lay them over 16-byte aligned LDS");

// what `decide` leaves in the registers of its wave for `list`
struct Listed {
    unsigned long long ranked;  // the lanes whose agents take the rank path
    int xl;                     // the list
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// inclusive prefix sum over the 64 lanes (DPP row shifts and row broadcasts)
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return v;
}

// `decide`, by ONE whole wave: lane l holds agent a0 + l -- its pose, `live` (the slot has an agent), its checkpoint headers of
// the two sets (h0: cp_hdr[i], h1: cp_hdr[W A + i]; anything for a dead slot) and its group's fallback streak (rk_streak[i / 32]);
// `in`: what every lane reads of the world.  All of it can be asked for long before the call: nothing in here waits for a load.
// Which XCD's list the half appends to is dealt (rank_cand.hpp deal_list) by world-block w * HALVES + half; the caller runs on the
// XCD that the step's other kernels keep the world on (workgroup b on XCD b % 8).
struct WorldIn {
    float4 bbox;     // road_bbox[w]
    int r0, r1;      // road_off[w], road_off[w + 1]
    int selections;  // rk_hist[513]
};
__device__ __forceinline__ WorldIn world_in(const DevSim &d, int w) {
    WorldIn in;
    in.bbox = d.road_bbox[w];
    in.r0 = d.road_off[w]; in.r1 = d.road_off[w + 1];
    in.selections = d.rk_hist[513];
    return in;
}
template <int A_T>
__device__ __forceinline__ Listed decide_half(const DevSim &d, int w, int a0, int lane, float ex, float ey, float iw, float iz, bool live,
                                              float4 h0, float4 h1, int streak, const WorldIn &in, Half &s) {
#pragma clang fp contract(off)
    constexpr int HALVES = A_T / 64;
    const int blk = w * HALVES + a0 / 64;
    Listed out;
    out.ranked = 0ull;
    // which XCD's list this half appends to: dealt, so that every list gets the same mix of worlds when scenes repeat with a
    // period (rank_cand.hpp deal_block, deal_list)
    out.xl = d.rk_scan_rows ? (blk & 7) : rank_cand::deal_list(blk, d.W * HALVES);
    if (blk == 0 && lane == 0) d.rk_hist[GD_RH_ROWS] = 0;  // k_knn_order counts this selection's rows (gd_stat 22)
    const size_t i = (size_t)w * A_T + a0 + lane;
    const int r0 = in.r0;
    const int R = in.r1 - r0;
    int ncp = 0;
    bool own_cp = false, copy = false;
    // (every lane's own checkpoint headers first, published: an agent without a usable bound of its own borrows one below)
    if (!live) { h0 = make_float4(0.f, 0.f, __int_as_float(0), 0.f); h1 = h0; }
    s.hdr[lane] = h0;
    wave_sync();
    if (live) {
        const int grp = (int)(i / 32);
        const Decision o = decide(lane, ex, ey, iw, iz, h0, h1, in.bbox, s.hdr, R, K, d.p.observationRadius,
                                  d.rk_min_roads, d.rk_max_roads, streak, in.selections, grp, d.rk_scan_rows != 0);
        if (o.kind == FAR) {
            // every road is beyond the radius: radiusFilter leaves nothing (src/knn.hpp:83-97, 156-157).  No replay, no
            // checkpoints; the (empty) hand-over to k_map_rows is written here
            d.sel_hdr[i * 2] = make_float4(ex, ey, iw, iz);
            d.sel_hdr[i * 2 + 1] = make_float4(__int_as_float(0), __int_as_float(r0), 0.f, 0.f);
            d.cp_hdr[i] = make_float4(ex, ey, __int_as_float(0), 0.f);
        } else if (o.kind == FALLBACK) {
            d.rk_fallback[i / 32] = 1;
        } else if (o.kind == AFRESH) {
            // the waves of the workgroup bound it afresh (`rows`).  Round 3 sent such an agent's group to the history replay on keys.
            ncp = -1;
            s.p0[lane] = ex; s.p1[lane] = ey; s.p2[lane] = o.margin;
        } else if (o.kind == OWN) {
            ncp = o.n_cp;
            own_cp = true;
            d.rk_rec[i] = make_float4(o.move, o.margin, __int_as_float(own_record_bits(o)), 0.f);
        } else {
            // a donor's checkpoints (the wave that ranks the donor overwrites them during the ranking launch), or every row
            // (GPUDRIVE_RANK_SCAN_ROWS): copied into the agent's row by `rows`
            ncp = o.n_cp;
            copy = true;
            s.p0[lane] = o.move; s.p1[lane] = __int_as_float((o.donor >= 0 ? o.donor : lane) | o.set << 8); s.p2[lane] = o.margin;
        }
        d.rk_n[i] = o.state;
        d.rk_ticket[i] = o.reason;  // k_knn_rank takes a ticket (>= 0) once the agent's ranks exist; < -1: why it fell back
    }
    s.ncp[lane] = own_cp ? 0 : ncp;
    {
        // published once: the waves of `rows` must all see ONE mask (a wave that finishes an agent rewrites its ncp entry, and a
        // late reader of it would deal the turns differently and skip the barrier behind the loop)
        const unsigned long long nd = __ballot(ncp < 0), cp = __ballot(copy);
        if (lane == 0) {
            s.needy[0] = (unsigned int)nd; s.needy[1] = (unsigned int)(nd >> 32);
            s.copied[0] = (unsigned int)cp; s.copied[1] = (unsigned int)(cp >> 32);
        }
    }
    if (ncp < 0) ncp = 1;  // (bounded afresh: on the rank path like the others)
    // the agents on the rank path, as a list: k_knn_rank's waves share THEM out, not the live agents (on the Waymo tiles
    // five agents in six are parked out of reach of every road, and a wave that drew three of the others set the pace).
    // One list per XCD (dealt: `xl` above; k_knn_rank's waves take the list of their own XCD, so an agent's
    // road points are gathered into the L2 that scanned them, and eight counters are asked instead of one: a thousand
    // workgroups adding to one address at once cost the kernel 10 us)
    out.ranked = __ballot(ncp > 0);
    return out;
}

// `list`, by the wave of `decide` with what that returned
template <int A_T>
__device__ __forceinline__ void list_half(const DevSim &d, int w, int a0, int lane, const Listed &l) {
    if (l.ranked == 0ull) return;
    const size_t WA = (size_t)d.W * A_T;
    int base = 0;
    if (lane == 0) base = atomicAdd(&d.rk_hist[528 + l.xl], __popcll(l.ranked));
    base = __builtin_amdgcn_readfirstlane(base);
    if ((l.ranked >> lane) & 1ull) {
        // bounds audit (engine.hpp GD_RANK_AUDIT): a list cursor outside the list is counted and clamped into it
        int at = base + __popcll(l.ranked & ((1ull << lane) - 1ull));
        if ((unsigned int)at >= (unsigned int)WA) {
            atomicAdd(&d.rk_hist[GD_RANK_AUDIT], 1);
            at = at < 0 ? 0 : (int)WA - 1;
        }
        d.rk_list[(size_t)l.xl * WA + at] = (int)((size_t)w * A_T + a0 + lane);
    }
}

// whether `rows` has anything to do for the half (workgroup-uniform once a workgroup barrier lies behind `decide`)
__device__ __forceinline__ bool rows_needed(const Half &s) { return (s.needy[0] | s.needy[1] | s.copied[0] | s.copied[1]) != 0u; }

// `rows`, by a workgroup of 256 threads (every thread calls, after a workgroup barrier behind `decide`; rows_needed holds).
// When the call returns every wave is done with both pieces of LDS.
template <int A_T>
__device__ __forceinline__ void rows_half(const DevSim &d, int w, int a0, Half &s, Rows &b) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t WA = (size_t)d.W * A_T;
    const int r0 = d.road_off[w];
    const int R = d.road_off[w + 1] - r0;
    const unsigned long long needy = (unsigned long long)s.needy[0] | (unsigned long long)s.needy[1] << 32;
    const unsigned long long copied = (unsigned long long)s.copied[0] | (unsigned long long)s.copied[1] << 32;
    // ---- copied rows: lane l of the first wave walks the checkpoints that bound agent a0 + l ----
    if (wave == 0 && ((copied >> lane) & 1ull)) {
        const size_t i = (size_t)w * A_T + a0 + lane;
        const float move = s.p0[lane], margin = s.p2[lane];
        const int from = __float_as_int(s.p1[lane]), set = from >> 8;
        const size_t src = (size_t)w * A_T + a0 + (from & 255);  // the agent whose checkpoint rows bound this selection
        const int ncp = s.ncp[lane];
        float t = 1.f;
        const unsigned short *cr = d.cp_road + ((size_t)set * WA + src) * NCP;
        const float *ct = d.cp_T + ((size_t)set * WA + src) * NCP;
        unsigned int fmax = 0u;  // (rank_cand.hpp: with the running maximum "in force" is a count of entries)
        for (int q = 0; q < ncp; q++) {
            t = ct[q];
            fmax = rank_cand::running_max(fmax, cr[q]);
            b.first[q][lane] = (unsigned short)fmax;
            b.thr[q][lane] = rank_cand::cp_threshold(t, move, margin);  // (an unusable entry bounds nothing)
        }
        d.rk_rec[i] = make_float4(move, t, __int_as_float(ncp | GD_RK_REC_ROW), 0.f);  // t: the last K-th key, scales the ranking buckets
    }
    // ---- agents without a usable bound: one wave each streams the world's roads once, in scan order, and keeps a histogram of
    // their squared distances (16 buckets per octave: the exponent and four mantissa bits).  At up to 39 road counts spaced
    // geometrically (the K-th distance falls like the logarithm of the roads seen) the upper edge of the bucket that holds the
    // K-th smallest distance so far is a bound of the K-th distance from there on -- a checkpoint like those a previous
    // selection leaves, at most 4.4 % loose, made without one.  About 6 us per such agent. ----
    if (needy != 0ull) {  // (workgroup-uniform)
        constexpr int BASE = (127 - 2) << 4;  // bucket 0: below 2^-2 m^2; bucket 255: 2^13.9 m^2 (118 m) and beyond = unbounded
        unsigned int *hist = b.hist[wave];
        int turn = 0;
        for (unsigned long long rest = needy; rest != 0ull; rest &= rest - 1ull, turn++) {
            if ((turn & 3) != wave) continue;  // wave-uniform
            const int al = __ffsll((long long)rest) - 1;
            const float bx = s.p0[al], by = s.p1[al], mg = s.p2[al];
#pragma unroll
            for (int k = 0; k < 4; k++) hist[k * 64 + lane] = 0u;
            if (lane == 0) { b.first[0][al] = (unsigned short)((K / 32) * 32); b.thr[0][al] = __builtin_inff(); }
            const float ratio = exp2f(log2f(fmaxf((float)R / 256.f, 1.f)) / (float)(NCP - 2));
            float pf = 256.f, tlast = __builtin_inff();
            int pq = 256, q = 1;
            float2 nxt = lane < R ? d.road_xy[r0 + lane] : make_float2(0.f, 0.f);
            for (int rb = 0; rb < R; rb += 64) {
                const float2 xy = nxt;
                if (rb + 64 + lane < R) nxt = d.road_xy[r0 + rb + 64 + lane];
                if (rb + lane < R) {
                    const float dx = xy.x - bx, dy = xy.y - by;
                    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
                    atomicAdd(&hist[min(255, max(0, (int)(__float_as_uint(d2) >> 19) - BASE))], 1u);
                }
                if (rb + 64 == pq && q < NCP && pq < R) {  // wave-uniform: roads [0, pq) are in the histogram
                    wave_sync();
                    const uint4 h = reinterpret_cast<const uint4 *>(hist)[lane];  // lane l owns buckets 4 l .. 4 l + 3
                    const int own = (int)(h.x + h.y + h.z + h.w);
                    const int incl = wave_incl_scan(own), excl = incl - own;
                    int jb = 0, before = excl;
                    if (before + (int)h.x < K) { before += (int)h.x; jb = 1;
                        if (before + (int)h.y < K) { before += (int)h.y; jb = 2;
                            if (before + (int)h.z < K) { jb = 3; } } }
                    const unsigned long long cross = __ballot(excl < K && incl >= K);  // exactly one lane: pq >= 256 > K
                    const int Lc = __ffsll((long long)cross) - 1;
                    const int bucket = 4 * Lc + __builtin_amdgcn_readlane(jb, Lc);
                    const float T = bucket >= 255 ? __builtin_inff() : __uint_as_float((unsigned int)(bucket + 1 + BASE) << 19);
                    if (lane == 0) {
                        const float reach = sqrtf(T) * 1.0001f + 1e-3f;
                        float thr = reach * reach * 1.0001f * mg * 1.001f;  // (the squared distances here are the scan's own form)
                        if (!(thr >= 0.f)) thr = __builtin_inff();
                        b.first[q][al] = (unsigned short)min(pq, 65535);
                        b.thr[q][al] = thr;
                    }
                    tlast = T;
                    q++;
                    pf *= ratio;
                    pq = max(pq + 64, ((int)pf + 63) & ~63);
                }
            }
            if (lane == 0) {
                s.ncp[al] = q;
                // (the last K-th key scales the ranking buckets)
                d.rk_rec[(size_t)w * A_T + a0 + al] = make_float4(0.f, tlast < 1e30f ? tlast : 1.f, __int_as_float(q | GD_RK_REC_ROW), 0.f);
            }
        }
    }
    __syncthreads();
    // The checkpoint rows of the agents on the rank path, agent-major (k_knn_rank reads an agent's row as one coalesced
    // load), whole rows: the entries behind an agent's last checkpoint are never in force
    {
        unsigned short *rowf = d.rk_cpf + ((size_t)w * A_T + a0) * NCP;
        float *rowt = d.rk_cpt + ((size_t)w * A_T + a0) * NCP;
        for (int e = tid; e < 64 * NCP; e += 256) {
            const int ag = e / NCP, q = e - ag * NCP;
            if (q < s.ncp[ag]) {
                rowf[e] = b.first[q][ag];
                rowt[e] = b.thr[q][ag];
            }
        }
    }
    __syncthreads();  // (the caller may reuse the LDS)
}

}  // namespace rank_setup
}  // namespace gd
#endif
