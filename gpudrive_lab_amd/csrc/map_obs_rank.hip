// Road observations in the reference's row order, fast path: the heap history replayed on 16-bit RANKS.
//
// selectKNearestRoadEntities (reference src/knn.hpp:103-158) pushes every road that is closer than the running K-th
// distance through an SGI binary heap (src/binary_heap.hpp) and returns the heap ARRAY, so the output order depends
// on every insert that ever happened.  map_obs.hip replays that history on fp32 keys + u16 indices (1200 B of LDS per
// agent: 128 agents per CU, one lone wave per SIMD, two generations of workgroups at 1024 x 64).  The heap's
// behaviour depends only on the OUTCOME of key comparisons, so this file replays it on ranks:
//
//   the set-up +  The agent's CANDIDATES (set-up, rank_setup.hpp: one lane per agent, run by the state step k_world_step -- or by
//   k_knn_rank    k_knn_scan, a launch of its own, under GPUDRIVE_RANK_SCAN_KERNEL=1 -- who takes this path, and the row of checkpoints
//                 that bounds the agent's candidates; rank: one wave per agent, which culls the world's blocks of 16 roads
//                 against that row, scans the surviving blocks in index order and keys what passes: rank_cand.hpp): roads
//                 0..K-1 plus every later
//                 road whose key is below a bound that provably is not smaller than the K-th distance the heap holds when
//                 the reference reaches that road.  The bound comes from the previous selection of the same agent: the
//                 K-th smallest distance over a fixed prefix of roads is 1-Lipschitz in the agent's position, and the
//                 previous replay recorded it at checkpoints (every 32 candidates).  A road that is not a candidate fails
//                 the reference's `cmp(current, heap[0])` test (src/knn.hpp:138-143) and never touches the heap, so
//                 replaying the candidates alone reproduces the heap exactly; candidates that are not inserts fail the
//                 same test in the replay.  The candidates' exact keys (gd_math.hpp ego_dist2, the reference's
//                 arithmetic) are ranked: e = (number of candidates with a smaller key + 1) << 5 | (index among the
//                 candidates with an EQUAL key).  key_a < key_b  <=>  (e_a >> 5) < (e_b >> 5), equal keys compare
//                 equal like in the reference, and e still names the candidate.  400 B of heap per agent instead of 1200.
//   k_knn_replay  one lane per agent, 64 agents per wave, the heap as u16 pairs in LDS: make_heap, then
//                 pop_heap / push_heap per insert, statement for statement the reference's algorithm.
//   k_knn_finish  one wave per agent: ranks back to road indices, radiusFilter (src/knn.hpp:83-97), the checkpoints'
//                 K-th distances for the next step, hand-over to k_map_rows.
//
// An agent without a usable bound (first selection after the worlds were built, a logged agent that reappears somewhere else)
// borrows a neighbour's checkpoints or is bounded afresh inside k_knn_scan; one with more candidates than the standard
// ranking holds (1272) is ranked by the long-list instantiation (2552).  Only an agent beyond that, with more equal keys than
// a rank can count (32; long lists 16), or in a world with fewer than K roads (or below rk_min_roads) raises the fallback flag
// of its group of 32 agents; k_map_obs (map_obs.hip) then selects for that group as before -- the same rows by construction
// -- and records checkpoints, so the group is back on this path at the next step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "engine.hpp"
#include "gd_math.hpp"
#include "rank_cand.hpp"
#include "rank_heap.hpp"
#include "rank_setup.hpp"

namespace gd {

namespace {

constexpr int K = GD_MAP_OBS_K;
constexpr int CAP = GD_RANK_CAP;   // candidates per agent
constexpr int NCP = GD_RANK_NCP;   // checkpoints per agent
constexpr int SPL = GD_RANK_SPL;   // sorted slots handed to k_knn_finish
constexpr int KT = GD_RANK_KT;     // key table entries per agent
constexpr int TILE = 32;           // candidates between checkpoints (standard agents; long lists: 64)
// Two instantiations of the ranking.  The standard one takes up to CAP - 8 = 1272 candidates in 10 KB of LDS (sixteen waves
// per CU) and serves nearly every agent; an agent with more (unreduced Waymo polylines: 200 ln(R / 200) inserts and the
// superset on top, one agent in eight beyond 6,000 roads; fast agents late in an episode) is put on a list and ranked by
// the LONG instantiation afterwards: 2552 candidates, 20 KB, ranks of 12 + 4 bits instead of 11 + 5, a checkpoint every 64
// candidates so that their number still fits the 40 slots.  Round 3 sent such an agent's whole group of 32 to the history
// replay on keys (k_map_obs), at least a millisecond for the launch, and therefore kept worlds above 6,000 roads off the
// rank path altogether.
constexpr int CAP_LONG = GD_RANK_CAP_LONG;
template <int CAP_T>
struct RankGeo {
    static constexpr bool LONG = CAP_T > CAP;
    static constexpr int NG = CAP_T / 64;          // candidates per lane
    static constexpr int NMAX = CAP_T - 8;         // most candidates an agent is ranked with (room for the end markers)
    static constexpr int NB = CAP_T;               // ranking buckets
    static constexpr int NLIN = CAP_T * 3 / 5;     // of which linear in the key (up to 1.5 x the previous K-th key); the others take
    static constexpr int TSH = LONG ? 6 : 5;       // log2 (candidates between checkpoints)
    static constexpr int RSH = LONG ? 4 : 5;       // bits of a rank that count the equal keys before it
    static constexpr int KTN = LONG ? GD_RANK_KT_LONG : GD_RANK_KT;  // floats per key-table row
};
constexpr int NB = RankGeo<CAP>::NB;
                                   // the eight octaves above that, 64 each: about one candidate per bucket on either side
static_assert(K + (NCP - 1) * TILE >= CAP && K + (NCP - 1) * 64 >= CAP_LONG, "a checkpoint slot for every tile of candidates");
static_assert(CAP % 64 == 0 && NB % 128 == 0 && CAP < 2047 && CAP_LONG % 640 == 0 && CAP_LONG < 4095, "geometry; less + 1 fits 11 / 12 bits");
static_assert(SPL >= K + 31 && SPL <= CAP && KT >= CAP / 16 + 1, "every slot the finish looks up; an entry per 16 slots + the last");
constexpr int RK_FAR = rank_setup::RK_FAR;  // rk_n: no road of the world can be within the agent's radius
constexpr int RK_TIES = 1 << 30;   // rk_ticket: the agent took its place in the replay order, then fell back (equal keys)

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

// inclusive running maximum over the 64 lanes of non-negative values (the same steps; a lane without a source takes 0)
__device__ __forceinline__ int wave_incl_max_nonneg(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
    return v;
}

// Wave-wide max / min / sum on the same DPP steps (lane 63 of the inclusive scan, broadcast): a `__shfl_xor` butterfly is six
// dependent LDS-crossbar round trips, this is six vector instructions and a readlane.  Lanes without a source keep their own
// value, which is neutral for max and min.
#define GD_DPP_SELF(v, ctrl, rows) __builtin_amdgcn_update_dpp((v), (v), (ctrl), (rows), 0xf, false)
__device__ __forceinline__ int wave_max(int v) {
    v = max(v, GD_DPP_SELF(v, 0x111, 0xf));
    v = max(v, GD_DPP_SELF(v, 0x112, 0xf));
    v = max(v, GD_DPP_SELF(v, 0x114, 0xf));
    v = max(v, GD_DPP_SELF(v, 0x118, 0xf));
    v = max(v, GD_DPP_SELF(v, 0x142, 0xa));
    v = max(v, GD_DPP_SELF(v, 0x143, 0xc));
    return __builtin_amdgcn_readlane(v, 63);
}
// (non-negative floats order like their bit patterns)
__device__ __forceinline__ float wave_max_nonneg(float f) { return __int_as_float(wave_max(__float_as_int(f))); }
__device__ __forceinline__ float wave_min_nonneg(float f) { return __int_as_float(~wave_max(~__float_as_int(f))); }
__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_incl_scan(v), 63); }
// the active lanes for which `p` holds.  (__ballot goes through a compare of the predicate as an integer with 0, which costs a
// select and a compare per call where the predicate is a lane mask already)
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// set bits of a ballot below this lane's own (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ int bits_below_lane(unsigned long long b) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u));
}

// Scratch rows that one kernel writes once and the next reads once (checkpoint rows, ranks, heap arrays, tables): streaming
// (nt) accesses, so that they take no room from what the step reads again and again (the road arrays, the pose planes).
#ifndef GD_NT_FINISH_LOAD
#define GD_NT_FINISH_LOAD 1
#endif
#ifndef GD_NT_REPLAY_LOAD
#define GD_NT_REPLAY_LOAD 1
#endif
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ T stream_load(const T *p) { return __builtin_nontemporal_load(p); }
template <typename T>
__device__ __forceinline__ void stream_store(T v, T *p) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ uint4 stream_load(const uint4 *p) {
    const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stream_store(uint4 v, uint4 *p) {
    u4v t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<u4v *>(p));
}
__device__ __forceinline__ uint2 stream_load(const uint2 *p) {
    const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(p));
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void stream_store(uint2 v, uint2 *p) {
    u2v t; t.x = v.x; t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<u2v *>(p));
}

// bounds audit (engine.hpp GD_RANK_AUDIT): `idx` must lie in [0, size); counts the violation and returns an index that does
__device__ __forceinline__ int audited(const DevSim &d, int idx, int size) {
    if ((unsigned int)idx < (unsigned int)size) return idx;
    atomicAdd(&d.rk_hist[GD_RANK_AUDIT], 1);
    return idx < 0 ? 0 : size - 1;
}

// key comparison on ranks: key(a) < key(b)  <=>  (a >> 5) < (b >> 5)  <=>  (a | 31) < b.  0 is "below everything".
// (tm: 31 for a standard agent's ranks, 15 for a long list's: RankGeo::RSH)
__device__ __forceinline__ bool rank_lt(unsigned int a, unsigned int b, unsigned int tm = 31u) { return (a | tm) < b; }

// ------------------------------------------------------------------------------------------------------------------
// k_knn_scan: the SET-UP of the selection (rank_setup.hpp) as a launch of its own, one workgroup (4 waves) per 64 agent slots
// of a world.  The state step runs the same text itself (kernels.hip, the FOLD instantiations of k_world_step) and the rank
// path then starts with k_knn_rank; this kernel is launched only under GPUDRIVE_RANK_SCAN_KERNEL=1 (A/B runs, twin tests).
// ------------------------------------------------------------------------------------------------------------------
template <int A_T>
__global__ __launch_bounds__(256) void k_knn_scan(DevSim d) {
    if (d.gate_any && *d.any_reset == 0) return;  // device-driven reset pass: nothing was flagged this step
    constexpr int HALVES = A_T / 64;
    const int w = blockIdx.x / HALVES, a0 = (blockIdx.x % HALVES) * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = d.shape[w * 2 + 0];
    __shared__ rank_setup::Half s_half;
    __shared__ rank_setup::Rows s_rows;
    rank_setup::Listed listed;
    if (wave == 0) {
        const size_t i = (size_t)w * A_T + a0 + lane, WA = (size_t)d.W * A_T;
        listed = rank_setup::decide_half<A_T>(d, w, a0, lane, d.px[i], d.py[i], d.qw[i], d.qz[i], a0 + lane < n, d.cp_hdr[i], d.cp_hdr[WA + i],
                                              d.rk_streak[i / 32], rank_setup::world_in(d, w), s_half);
    }
    __syncthreads();
    if (rank_setup::rows_needed(s_half)) rank_setup::rows_half<A_T>(d, w, a0, s_half, s_rows);  // (workgroup-uniform)
    if (wave == 0) rank_setup::list_half<A_T>(d, w, a0, lane, listed);
}

// ------------------------------------------------------------------------------------------------------------------
// k_knn_rank: one wave per live agent.  Checkpoint row -> candidate list with exact keys (rank_cand.hpp: the blocks of 16
// consecutive roads that cannot hold a candidate are culled, a lane per block; the surviving blocks are scanned in index
// order, four per pass, coalesced), ranks.
// ------------------------------------------------------------------------------------------------------------------
// 10 KB of LDS per agent, so that sixteen waves fit a CU: the kernel is a chain of LDS and memory round trips, and with two
// waves per SIMD (20 KB) it waited 46 % of its cycles (profiles/r03: SQ_WAIT_ANY).  A lane keeps its up to 20 candidates
// (positions lane, lane + 64, ...) in registers through all passes; LDS holds only what lanes exchange.
template <int CAP_T>
struct RankLds {
    union {
        struct {
            float ckey[CAP_T];            // the candidates' exact keys and ...
            unsigned short cidx[CAP_T];   // ... road indices in road order, while the scan hands them to their lanes
        } c;
        struct {
            float skey[CAP_T];            // the keys in bucket order
            unsigned short spos[CAP_T];   // bucket order -> candidate position
        } s;
        unsigned short spc[CAP_T];        // at the end: sorted slot -> road index
    };
    // bucket counters, two u16 per word; then cursors: after the scatter the END of each bucket.  Idle until the bucket
    // counts, so the cull and the scan keep their tables here: the surviving blocks (block | checkpoints at or before it << 10,
    // ascending) and the thresholds by that count (entry 0: unbounded)
    unsigned int cnt2[RankGeo<CAP_T>::NB / 2];
};
static_assert(sizeof(RankLds<CAP>) <= 10240 && sizeof(RankLds<CAP_LONG>) <= 20480, "sixteen / eight waves per CU");
constexpr int LSTN = (GD_MAX_ROAD_ENTITIES + GD_LIN_BLK - 1) / GD_LIN_BLK + 15;  // blocks of the largest world, rounded to a multiple of 4 below
constexpr int LSTN4 = (LSTN + 3) & ~3;
static_assert(LSTN4 <= 1024 && NCP < 64 && rank_cand::CHUNK % GD_LIN_BLK == 0 && 64 % GD_LIN_BLK == 0, "block and count share 16 bits; a block inside one chunk; whole blocks per pass");
constexpr size_t CAND_TABLES = LSTN4 * sizeof(unsigned short) + (NCP + 2) * sizeof(float);  // (+ the last K-th key behind the thresholds)
static_assert(CAND_TABLES <= sizeof(RankLds<CAP>::cnt2) && CAND_TABLES <= sizeof(RankLds<CAP_LONG>::cnt2), "the tables fit the idle counters of both instantiations");
// the cull's table of checkpoints per 32-road chunk (rank_cand.hpp cp_table): entries per lane in the largest world; the scatter's
// targets (u32) and the table itself (count, reach) side by side in the candidate keys' buffer
constexpr int CP_EPL = ((GD_MAX_ROAD_ENTITIES + rank_cand::CHUNK - 1) / rank_cand::CHUNK + 63) / 64;
static_assert(64 * CP_EPL * (sizeof(unsigned int) + sizeof(uint2)) <= sizeof(float) * CAP, "the chunk table fits the candidate keys of both instantiations");

// What the ranking of one agent reads from global memory before it can start, fetched while the previous agent of the
// wave is being ranked (the fetches are a chain of dependent loads, several microseconds end to end).
struct RankIn {
    int i, state, r0, R, b0, li;  // li: the entry of the list this agent came from (a long list's scratch rows go by it)
    float ex, ey, iw, iz;
    // lane q below the number of checkpoints: checkpoint q of the agent; the other lanes: never in force.  With a row (rec_pack &
    // GD_RK_REC_ROW): the entry of k_knn_scan's row, first road (running maximum) and threshold.  Without: the agent's own
    // cp_road / cp_T entry as recorded; rank_agent makes the row's entry of it (rec_move, the margin in rec_y)
    unsigned int cfirst;
    float cthr;
    // k_knn_scan's record (engine.hpp rk_rec): how far the agent is from where its checkpoints were recorded; the margin (no row)
    // or the last K-th key of the row; checkpoints | set << 8 (no row) or checkpoints | GD_RK_REC_ROW
    float rec_move, rec_y;
    int rec_pack;
};
// A value at a wave-uniform address that this kernel does not change, read through the scalar cache.  As vector loads the
// chain list -> agent -> state / pose waited, at each link, for every store the wave had issued for the previous agent
// (vector memory operations are counted in order): a fifth of the kernel.
// INVARIANT (nothing enforces it but the call sites below): the scalar cache is not coherent with this kernel's own vector
// stores, so an address read through here must never be read AFTER any wave of the same launch has written it.  What is
// read this way: arrays written by EARLIER kernels only (rk_list, rk_hist[528..], rk_rec, road_off, blk_off, the pose planes: the
// scalar cache is invalidated at every kernel boundary), and rk_n[i] -- which this kernel does rewrite, but only the wave
// that ranks agent i writes rk_n[i], and it reads it (rank_fetch) before it writes it (end of rank_agent); a cache line
// shared with another agent's already rewritten entry may be stale for THAT entry, which this wave never looks at.
template <typename T>
__device__ __forceinline__ T uniform_load(const T *p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) T *>(reinterpret_cast<uintptr_t>(p));
}
template <int A_T>
__device__ __forceinline__ RankIn rank_fetch(const DevSim &d, const int *list, int li, int count, int lane) {
    RankIn in;
    in.li = li;
    in.i = li < count ? uniform_load(list + li) : 0;
    in.state = li < count ? uniform_load(d.rk_n + in.i) : 0;  // (k_knn_scan's; this kernel rewrites it once the agent is ranked)
    const int w = in.i / A_T;
    in.r0 = uniform_load(d.road_off + w);
    in.R = uniform_load(d.road_off + w + 1) - in.r0;
    in.ex = uniform_load(d.px + in.i); in.ey = uniform_load(d.py + in.i);
    in.iw = uniform_load(d.qw + in.i); in.iz = -uniform_load(d.qz + in.i);  // the INVERSE rotation
    in.b0 = uniform_load(d.blk_off + w);
    // (k_knn_scan's record: written by the earlier kernel only, so the invariant above holds)
    const float *rec = reinterpret_cast<const float *>(d.rk_rec + in.i);
    in.rec_move = uniform_load(rec); in.rec_y = uniform_load(rec + 1); in.rec_pack = __float_as_int(uniform_load(rec + 2));
    // Lane q reads entry q of the agent's checkpoints, two coalesced loads from wave-uniform bases: of the row k_knn_scan wrote
    // (rk_cpf / rk_cpt), or of the agent's own checkpoints where the previous selection (set 0) or the episode's first (set 1)
    // left them.  Set 0's first roads are rewritten during this launch, by this wave alone, in the ranking of this agent:
    // behind this read.  (Other agents' rows of cp_road must not be read here: their waves may have rewritten them.)
    const bool has_row = (in.rec_pack & GD_RK_REC_ROW) != 0;
    const size_t own = ((size_t)((in.rec_pack >> 8) & 1) * d.W * A_T + in.i) * NCP, row = (size_t)in.i * NCP;
    const unsigned short *pf = has_row ? d.rk_cpf + row : d.cp_road + own;
    const float *pt = has_row ? d.rk_cpt + row : d.cp_T + own;
    in.cfirst = rank_cand::NO_CP;
    in.cthr = __builtin_inff();
    if (in.state == 1 && lane < min(in.rec_pack & 0xff, NCP)) {
        in.cfirst = pf[(unsigned int)lane];
        in.cthr = pt[(unsigned int)lane];
    }
    return in;
}

#ifdef GD_CLOCKS
// builds with -DGD_CLOCKS (tools/build_expt.sh clk -DGD_CLOCKS; nothing else differs from the product code): clock ticks per
// phase of the ranking, summed per wave in scalar registers, added up over the waves (gd_stat 10..17)
struct PhaseClock {
    unsigned int prev, sum[8];
    __device__ __forceinline__ void mark(int n) {
        const unsigned int t = (unsigned int)__builtin_amdgcn_s_memtime();
        sum[n] += t - prev;
        prev = t;
    }
};
#define GD_PHASE(n) clk.mark(n)
#else
struct PhaseClock {};
#define GD_PHASE(n)
#endif
// A wave asks its list's cursor for the entry it ranks next (lane 0; the answer is lane 0's, taken with readfirstlane).  The
// cursor changes during the launch: it is read through the atomic's return only, never through uniform_load (INVARIANT above).
__device__ __forceinline__ int rank_draw(int *cursor, int lane) {
    int e = 0;
    if (lane == 0) e = atomicAdd(cursor, 1);
    return e;
}
template <int A_T, int CAP_T>
__device__ __forceinline__ void rank_agent(const DevSim &d, const RankIn &in, int lane, RankLds<CAP_T> &L, PhaseClock &clk, int drawn,
                                           int count, const int *list, RankIn &nxt) {
    using G = RankGeo<CAP_T>;
    constexpr int NB = G::NB, NLIN = G::NLIN, NMAX = G::NMAX;
    constexpr unsigned int TM = (1u << G::RSH) - 1u;  // most equal keys before a candidate that its rank can count
    if (__builtin_amdgcn_readfirstlane(in.state) != 1) {  // fallback or too far from every road (k_knn_scan)
        nxt = rank_fetch<A_T>(d, list, __builtin_amdgcn_readfirstlane(drawn), count, lane);
        return;
    }
    // every lane fetched the same values: as scalars they index through scalar base addresses (a per-lane 64-bit pointer per
    // array costs two registers each, and reloading a spilled one made the wave wait for all its outstanding stores)
    auto uni = [](int v) -> int { return __builtin_amdgcn_readfirstlane(v); };
    auto unif = [](float v) -> float { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    const int i = uni(in.i), r0 = uni(in.r0), R = uni(in.R);
    const int group = i / 32;  // 32 consecutive agent slots of a world: the fallback unit (a workgroup of k_map_obs)
    constexpr int NG = G::NG;  // candidates per lane

    const float ex = unif(in.ex), ey = unif(in.ey), iw = unif(in.iw), iz = unif(in.iz);
    // ---- CULL (rank_cand.hpp): lane l takes block b0 + l of the world's road blocks (GD_LIN_BLK consecutive roads inside a
    // circle, engine.hpp road_blk) and drops it if no road of it can be a candidate under the checkpoint in force for it; the
    // survivors are listed in ascending order, one ballot per 64 blocks = 1024 roads.  The checkpoint in force comes from a
    // table built once per agent (rank_cand.hpp cp_table): lane q holds checkpoint q of the row and leaves q + 1 in the entry
    // of the first chunk it is in force for, a running maximum over the chunks (each lane on consecutive entries, a DPP
    // max-scan across the lanes) carries it on, and every chunk gets (checkpoints at or before it, the reach of the last of
    // them).  The table lives in the candidate buffer, which nothing else uses until the scan stores its first candidate. ----
    unsigned short *const lst = reinterpret_cast<unsigned short *>(L.cnt2);
    float *const tthr = reinterpret_cast<float *>(L.cnt2) + LSTN4 / 2;  // threshold by checkpoints at or before: 0 = unbounded
    unsigned int cfirst = in.cfirst;
    float cthr = in.cthr, t_last_in = unif(in.rec_y);  // (with a row: the last K-th key)
    if (!(uni(in.rec_pack) & GD_RK_REC_ROW)) {
        // the agent's own checkpoints as recorded (rank_fetch): the row k_knn_scan would have made of them -- the threshold by
        // the shared rule, the first road as the running maximum over the entries before it, nothing behind the last one
        const int n_own = min(uni(in.rec_pack) & 0xff, NCP);  // 1 .. NCP
        const bool have = lane < n_own;
        t_last_in = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cthr), n_own - 1));  // the last K-th key
        const unsigned int fmax = (unsigned int)wave_incl_max_nonneg(have ? (int)cfirst : 0);  // (16-bit road indices)
        cthr = have ? rank_cand::cp_threshold(cthr, unif(in.rec_move), unif(in.rec_y)) : __builtin_inff();
        cfirst = have ? fmax : rank_cand::NO_CP;
    }
    // (behind the thresholds: the last K-th key, kept here for the refill, not in a register)
    if (lane <= NCP) tthr[lane + 1] = lane < NCP ? cthr : t_last_in;
    if (lane == 63) tthr[0] = __builtin_inff();
    const float creach = rank_cand::block_reach(cthr);  // (lanes from NCP on: +inf, which is also what "no checkpoint" reads)
    const int nblk = (R + GD_LIN_BLK - 1) / GD_LIN_BLK;
    const int nch = rank_cand::chunks_of(R), epl = (nch + 63) >> 6;  // entries per lane: wave-uniform, at most CP_EPL
    unsigned int *const tmax = reinterpret_cast<unsigned int *>(L.c.ckey);  // [64 * CP_EPL] the scatter's targets
    uint2 *const tcp = reinterpret_cast<uint2 *>(L.c.ckey + 64 * CP_EPL);   // [64 * CP_EPL] per chunk: (count, reach)
#pragma unroll
    for (int u = 0; u < CP_EPL; u++)
        if (u < epl) tmax[u * 64 + lane] = 0u;
    wave_sync();
    if (lane < NCP && rank_cand::cp_table_takes(cfirst, nch)) atomicMax(&tmax[rank_cand::cp_table_chunk(cfirst)], rank_cand::cp_table_entry(lane));
    wave_sync();
    {
        int own[CP_EPL], run = 0;
#pragma unroll
        for (int u = 0; u < CP_EPL; u++) own[u] = u < epl ? (int)tmax[lane * epl + u] : 0;
#pragma unroll
        for (int u = 0; u < CP_EPL; u++) { run = max(run, own[u]); own[u] = run; }
        // the largest entry of the lanes below this one: the inclusive scan, taken from the lane before
        const int before = __builtin_amdgcn_ds_bpermute(((lane - 1) & 63) << 2, wave_incl_max_nonneg(run));
#pragma unroll
        for (int u = 0; u < CP_EPL; u++)
            if (u < epl) {
                const int cnt = lane ? max(own[u], before) : own[u];
                // the reach of checkpoint cnt - 1; none: lane 63's, +inf
                const int reach = __builtin_amdgcn_ds_bpermute(((cnt - 1) & 63) << 2, __float_as_int(creach));
                tcp[lane * epl + u] = make_uint2((unsigned int)cnt, (unsigned int)reach);
            }
    }
    wave_sync();
    const float4 *blk = d.road_blk + uni(in.b0);
    int nsv = 0;
    constexpr int CU = 4;  // batches of 64 blocks requested together
#pragma clang loop unroll(disable)
    for (int b0 = 0; b0 < nblk; b0 += 64 * CU) {
        float4 c[CU];
        uint2 cp[CU];
#pragma unroll
        for (int u = 0; u < CU; u++) {
            const int bc = min(b0 + u * 64 + lane, nblk - 1);
            c[u] = blk[(unsigned int)bc];
            cp[u] = tcp[rank_cand::chunk_base_of_block(bc, GD_LIN_BLK) / rank_cand::CHUNK];
        }
        // (all requested here, together: left alone the compiler sinks a batch's load into the per-lane branch it makes of the test)
        static_assert(CU == 4, "operand list");
        asm volatile("" : "+v"(c[0].x), "+v"(c[0].y), "+v"(c[0].z), "+v"(c[1].x), "+v"(c[1].y), "+v"(c[1].z), "+v"(c[2].x), "+v"(c[2].y), "+v"(c[2].z),
                     "+v"(c[3].x), "+v"(c[3].y), "+v"(c[3].z));
#pragma unroll
        for (int u = 0; u < CU; u++) {
            const int bb = b0 + u * 64;
            if (bb < nblk) {  // wave-uniform
                const int b = bb + lane;
                const bool sv = b < nblk && rank_cand::block_survives(b, GD_LIN_BLK, K, c[u].x, c[u].y, c[u].z, ex, ey, __uint_as_float(cp[u].y));
                const unsigned long long m = wave_ballot(sv);
                const int upto = nsv + __popcll(m);
                // (bounds audit, wave-uniform: the list holds a block of the largest world each, so this never happens)
                if (upto <= LSTN4) {
                    if (sv) lst[nsv + bits_below_lane(m)] = (unsigned short)((unsigned int)b | cp[u].x << 10);
                    nsv = upto;
                } else if (lane == 0) {
                    atomicAdd(&d.rk_hist[GD_RANK_AUDIT], 1);
                }
            }
        }
    }
    wave_sync();
    // the next agent's entry (rank_draw, asked for before the table): vector memory answers in order, so the cull's blocks
    // above waited for it too; from here on it is a scalar
    const int next_entry = uni(drawn);
    // ---- SCAN of the surviving blocks, four per pass (a quarter of the wave each), in index order: the per-road test
    // (rank_cand.hpp: k_knn_scan's former expression, bit for bit), the exact key (gd_math.hpp ego_dist2: the reference's
    // arithmetic), one ballot per pass; (road, key) go to LDS at the candidate's position.  Roads 0..K-1 are candidates
    // regardless and their blocks always survive, so the first K positions are their indices.  Writes stop at the buffer's
    // end, the count goes on.
    // A pass of the main loop holds only the per-road work.  Every pass but the last has four listed blocks, none of them the
    // world's last (the list ascends), so every road of theirs exists and nothing is clamped per lane; the loop takes four such
    // passes per trip, straight-line, while the buffer has room for all their roads (one wave-uniform test per trip), with the
    // list entries read a stage ahead of the thresholds and roads they select (stages of PB passes: entries, then threshold +
    // road, then test + key).  What is left -- up to four passes with the last one, partial or with the world's partial last
    // block; all the rest of an agent whose candidates may overflow the buffer -- goes through a guarded copy. ----
    int nin = 0;
    {
        // (PB passes requested together.  Measured at 1024 x 64, one run of 150 steps each, k_knn_rank with PB = 2: 420 us,
        // 4: 422, 8: 431 -- the scan does not wait for its own loads)
        constexpr int BPP = 64 / GD_LIN_BLK, PB = 2;  // blocks per pass
        const int np = (nsv + BPP - 1) / BPP, nfast = np - 1;  // passes; of them with four listed blocks that are not the world's last
        const int sub = lane / GD_LIN_BLK, o = lane % GD_LIN_BLK;
        const float2 *rxy = d.road_xy + r0;
        auto store = [&](bool cand, int r, float key, unsigned long long m, bool guard) {
            const int pos = nin + bits_below_lane(m);
            if (cand && (!guard || pos < CAP_T)) {
                L.c.cidx[pos] = (unsigned short)r;
                L.c.ckey[pos] = key;
            }
            nin += __popcll(m);
        };
        int p = 0;
        if (nfast >= 2 * PB) {
            // (the list is read as words of two entries and a lane takes its half with a bit-field extract: a 16-bit value carried
            // round the loop made the compiler shift it with SDWA forms, whose shift counts it kept in two vector registers from
            // the kernel's first instruction to its last -- five more spilled registers in the ranking behind this)
            const unsigned int *lsub = reinterpret_cast<const unsigned int *>(L.cnt2) + sub / 2;
            const unsigned int sh = (unsigned int)(sub & 1) * 16u;
            const unsigned int o8 = (unsigned int)o * (unsigned int)sizeof(float2);
            static_assert(BPP == 4, "two words per pass");
            struct Ents { unsigned int e[PB]; };
            struct Batch { unsigned int off[PB]; float thr[PB]; float2 xy[PB]; };
            auto entries = [&](Ents &en, int p0) {  // (a stage beyond the last full pass reads that pass again and is never taken)
#pragma unroll
                for (int u = 0; u < PB; u++) en.e[u] = lsub[min(p0 + u, nfast - 1) * (BPP / 2)];
            };
            auto issue = [&](Batch &bt, const Ents &en) {
#pragma unroll
                for (int u = 0; u < PB; u++) {  // the road's byte offset in the world's points: below 2^20, a scalar base + 32 bits
                    bt.off[u] = __builtin_amdgcn_ubfe(en.e[u], sh, 10u) * (unsigned int)(GD_LIN_BLK * sizeof(float2)) + o8;
                    bt.thr[u] = tthr[__builtin_amdgcn_ubfe(en.e[u], sh + 10u, 6u)];
                    bt.xy[u] = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(rxy) + bt.off[u]);
                }
            };
            auto take = [&](const Batch &bt) {
#pragma unroll
                for (int u = 0; u < PB; u++) {
                    const int r = (int)(bt.off[u] / (unsigned int)sizeof(float2));
                    __builtin_assume(r >= 0 && r < R);
                    const bool cand = rank_cand::is_candidate(r, K, R, bt.xy[u].x, bt.xy[u].y, ex, ey, bt.thr[u]);
                    store(cand, r, ego_dist2(ex, ey, iw, iz, bt.xy[u].x, bt.xy[u].y), wave_ballot(cand), false);
                }
            };
            Ents ea, eb;
            Batch ba, bb;
            entries(ea, 0);
            entries(eb, PB);
            issue(ba, ea);
#pragma clang loop unroll(disable)
            for (; p + 2 * PB <= nfast && nin + 2 * PB * 64 <= CAP_T; p += 2 * PB) {
                issue(bb, eb);
                entries(ea, p + 2 * PB);
                take(ba);
                issue(ba, ea);
                entries(eb, p + 3 * PB);
                take(bb);
            }
        }
#pragma clang loop unroll(disable)
        for (; p < np; p += 2 * PB) {  // the guarded copy: every index clamped, the writes stop at the buffer's end
            int r[2 * PB];
            float thr[2 * PB];
            float2 xy[2 * PB];
#pragma unroll
            for (int u = 0; u < 2 * PB; u++) {
                r[u] = R; thr[u] = 0.f; xy[u] = make_float2(0.f, 0.f);
                if (p + u < np) {  // wave-uniform: a trip of this loop is mostly the one last pass
                    const int e = (p + u) * BPP + sub;
                    const unsigned int ent = lst[min(e, LSTN4 - 1)];
                    const bool on = e < nsv;
                    r[u] = on ? (int)(ent & 1023u) * GD_LIN_BLK + o : R;
                    thr[u] = tthr[on ? min((int)(ent >> 10), NCP) : 0];
                    xy[u] = rxy[(unsigned int)min(r[u], R - 1)];
                }
            }
#pragma unroll
            for (int u = 0; u < 2 * PB; u++) {
                if (p + u < np) {
                    const bool cand = rank_cand::is_candidate(r[u], K, R, xy[u].x, xy[u].y, ex, ey, thr[u]);
                    store(cand, r[u], ego_dist2(ex, ey, iw, iz, xy[u].x, xy[u].y), wave_ballot(cand), true);
                }
            }
        }
    }
    wave_sync();
    // The next agent's inputs are requested here, behind the last road loads of this one: vector memory operations complete
    // in order, so requested up front they (from HBM) were what every load of the scan then waited for.
    nxt = rank_fetch<A_T>(d, list, next_entry, count, lane);
    // ---- more candidates than this instantiation ranks: on to the long-list instantiation, or to the fallback ----
    {
        const int total = nin;
        // (NMAX = CAP - 8: the sorted key array ends in eight +inf entries that reads past a bucket's end run into.  Round 3
        // took up to CAP candidates; with exactly CAP there was no room for an end marker and the clamp that stood in for it
        // re-read the LAST entry of the last bucket, which is not necessarily its largest: a candidate of that bucket could
        // count a smaller key twice)
        if (total > NMAX) {
            if (lane == 0) {
                bool passed_on = false;
                if (!G::LONG && total <= RankGeo<CAP_LONG>::NMAX) {
                    const int slot = atomicAdd(&d.rk_hist[GD_RH_LONG], 1);
                    if (slot < d.rk_nlong) {  // (rk_n stays 1, the ticket -1: the long-list launch finds the agent as k_knn_scan left it)
                        d.rk_longlist[slot] = i;
                        passed_on = true;
                    }
                }
                if (!passed_on) {
                    d.rk_n[i] = 0;
                    d.rk_ticket[i] = -3;  // more candidates than the buffers hold
                    d.rk_fallback[group] = 1;
                }
            }
            return;
        }
    }
#ifdef GD_CLOCKS
    clk.sum[7] += (unsigned int)((nsv + 3) / 4) << 8;  // the wave's passes through the scan above (gd_stat 17)
#endif
    // the agent's place in the replay order (k_knn_order: most candidates first).  Taken now: the counter's
    // answer is a trip to the L2 and back that nothing has to wait for until the agent is done
    const int bin = 255 - min(255, (nin - K) / 5);
    int ticket = 0;
    if (lane == 0) ticket = bin << 20 | atomicAdd(&d.rk_hist[bin], 1);
    GD_PHASE(1);
    if (GD_DIAG_IS(d.rk_dbg, 1)) return;
    // where this selection's checkpoints start to apply (their K-th distances are filled in by k_knn_finish): checkpoint 0
    // is the heap of the first K roads (road indices below K are candidates regardless), checkpoint q the heap after
    // candidate K + 32 q - 1, which holds for every road behind that candidate; rounded up to whole 32-road chunks of the scan
    if (lane <= (nin - K) >> G::TSH) {
        const int road = (int)L.c.cidx[K - 1 + (lane << G::TSH)];
        d.cp_road[(size_t)i * NCP + lane] = (unsigned short)(lane ? min(65535, (road + 1 + 31) & ~31) : (K / 32) * 32);
    }
    // ---- refill: lane l takes the candidates at positions l, l + 64, ... (road index and key) from LDS into registers ----
    // A lane has 13 candidates on average, 20 at most.  They are read in groups of GQ with one wave-uniform guard per group;
    // inside a group every lane reads, and a lane whose position lies beyond the last candidate keeps road 0 and key 0 instead of
    // the stale entry it read (its values take part in the passes below but never in a count, a store or a rank)
    constexpr int GQ = 5;
    static_assert(NG % GQ == 0, "whole groups");
    const float kmax = d.radius_key_max;
    int ci[NG];
    float key[NG];
    const float t_last = unif(tthr[NCP + 1]);
    float split = (t_last > 0.f && t_last < 1e30f) ? t_last * 1.5f : 1.f;
    int nle = 0, nlow = 0;  // candidates inside the radius / below `split` (second count in the upper half)
    float kmax_seen = 0.f, kmin_seen = __builtin_inff();
#pragma unroll
    for (int g0 = 0; g0 < NG; g0 += GQ) {
#pragma unroll
        for (int u = 0; u < GQ; u++) { ci[g0 + u] = 0; key[g0 + u] = 0.f; }
        if (g0 * 64 < nin) {  // wave-uniform
            int v[GQ];
            float kv[GQ];
#pragma unroll
            for (int u = 0; u < GQ; u++) {  // (beyond nin: stale, dropped below)
                v[u] = (int)L.c.cidx[(g0 + u) * 64 + lane];
                kv[u] = L.c.ckey[(g0 + u) * 64 + lane];
            }
            // (the ten LDS reads of a group are issued together and are complete here: without this the compiler sank each read
            // into a per-lane branch on `on` below and kept key[] as one 32-register tuple that it copied at every group -- 624
            // spilled registers)
            static_assert(GQ == 5, "operand list");
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(kv[0]), "+v"(kv[1]), "+v"(kv[2]), "+v"(kv[3]), "+v"(kv[4]));
#pragma unroll
            for (int u = 0; u < GQ; u++) {
                const int g = g0 + u;
                const bool on = g * 64 + lane < nin;
                ci[g] = on ? v[u] : 0;
                key[g] = on ? kv[u] : 0.f;
                nle += ((on & (key[g] <= kmax)) ? 1 : 0) + ((on & (key[g] < split)) ? 1 << 16 : 0);
                kmax_seen = fmaxf(kmax_seen, key[g]);
                kmin_seen = fminf(kmin_seen, on ? key[g] : __builtin_inff());
            }
        }
    }
    wave_sync();  // the candidate buffer becomes the sorted arrays
    nle = wave_sum(nle);
    kmax_seen = wave_max_nonneg(kmax_seen);  // keys are sums of squares
    kmin_seen = wave_min_nonneg(kmin_seen);
    nlow = nle >> 16;
    nle &= 0xffff;
    GD_PHASE(2);
    if (GD_DIAG_IS(d.rk_dbg, 2)) return;

    // ---- ranks.  Counting sort into NB buckets (a monotone function of the key: linear up to 1.5 x the previous
    // K-th key, where most candidates lie, logarithmic beyond), then the exact order inside each bucket ----
    for (int b = lane; b < NB / 2; b += 64) L.cnt2[b] = 0u;
    wave_sync();
    // The previous K-th key says where the candidates are dense only while the agent is near where it was recorded.  After
    // a jump — fewer than a quarter of the candidates below `split` (all of them in a band far above it), or every one
    // below it (a logged agent back from the padding position, src/sim.cpp:333-343, with checkpoints recorded out there:
    // the whole world in bucket 0) — the buckets are linear between the smallest and the largest key instead: any
    // monotone function gives the same ranks, a poor one makes the order inside a bucket quadratic.
    const bool jumped = nlow * 4 < nin || nlow == nin;  // wave-uniform
    const float lin_lo = jumped ? kmin_seen : 0.f;
    const int nlin = jumped ? NB : NLIN;
    const float lin_scale = jumped ? (float)NB / fmaxf(kmax_seen - kmin_seen, 1e-30f) : (float)NLIN / split;
    if (jumped) split = __builtin_inff();
    const unsigned int split_bits = __float_as_uint(split);
    // above `split` the buckets are uniform in the key's bit pattern (i.e. logarithmic) up to the largest candidate key
    const float log_scale = (float)(NB - NLIN) / (float)(max(__float_as_uint(kmax_seen), split_bits + 1u) - split_bits + 1u);
    auto bucket_of = [&](float k) -> int {
        if (k < split) return min(nlin - 1, max(0, (int)((k - lin_lo) * lin_scale)));
        return NLIN + min(NB - NLIN - 1, (int)((float)(__float_as_uint(k) - split_bits) * log_scale));
    };
    // (the bucket rides in the upper half of the road-index register: registers decide how many waves a SIMD holds)
#pragma unroll
    for (int g = 0; g < NG; g++) {
        if (g * 64 < nin) {  // wave-uniform
            const int b = bucket_of(key[g]);
            ci[g] |= b << 16;
            if (g * 64 + lane < nin) atomicAdd(&L.cnt2[b >> 1], 1u << ((b & 1) * 16));
        }
    }
    wave_sync();
    {
        // exclusive prefix over the buckets: lane l owns buckets l * (NB / 64) .. (an even number of them: whole words)
        constexpr int WPB = NB / 64 / 2;
        static_assert(WPB * 128 == NB, "whole counter words per lane");
        unsigned int own[WPB];
        int sum = 0;
#pragma unroll
        for (int k = 0; k < WPB; k++) { own[k] = L.cnt2[lane * WPB + k]; sum += (int)(own[k] & 0xffffu) + (int)(own[k] >> 16); }
        int run = wave_incl_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < WPB; k++) {
            const int lo = run, hi = run + (int)(own[k] & 0xffffu);
            run = hi + (int)(own[k] >> 16);
            L.cnt2[lane * WPB + k] = (unsigned int)lo | (unsigned int)hi << 16;
        }
    }
    wave_sync();
    GD_PHASE(3);
    if (GD_DIAG_IS(d.rk_dbg, 3)) return;
#pragma unroll
    for (int g0 = 0; g0 < NG; g0 += GQ) {
        if (g0 * 64 < nin) {  // wave-uniform
            int sl[GQ];
#pragma unroll
            for (int u = 0; u < GQ; u++) {  // any order inside the bucket; idle lanes add nothing (to bucket 0)
                const int b = ci[g0 + u] >> 16, sh = (b & 1) * 16;
                const unsigned int one = (g0 + u) * 64 + lane < nin ? 1u << sh : 0u;
                sl[u] = (int)((atomicAdd(&L.cnt2[b >> 1], one) >> sh) & 0xffffu);
            }
#pragma unroll
            for (int u = 0; u < GQ; u++) {
                if ((g0 + u) * 64 + lane < nin) {
                    L.s.skey[sl[u]] = key[g0 + u];
                    L.s.spos[sl[u]] = (unsigned short)((g0 + u) * 64 + lane);
                }
            }
        }
    }
    wave_sync();
    GD_PHASE(4);
    if (GD_DIAG_IS(d.rk_dbg, 4)) return;
    const unsigned short *cur16 = reinterpret_cast<const unsigned short *>(L.cnt2);  // cursor of bucket b = its END
    // Candidates with a smaller key = those of the earlier buckets + the smaller ones of the own bucket.  The pass is a chain
    // of LDS round trips with little to issue in between, so it reads generously: the first six members of every bucket at
    // once (most hold one or two), then four more per trip while any lane's bucket has members left.  Only keys are read;
    // candidates that met their own key more than once (equal keys, rare) get their place among those afterwards.
    // (a candidate's rank e replaces its bucket in the upper half of the road-index register: registers decide how many
    // waves a SIMD holds)
    unsigned int eqmask = 0u;  // bit g: candidate g of this lane shares its key with another candidate
    float *const kt_row = G::LONG ? d.rk_kt_long + (size_t)uni(in.li) * G::KTN : d.rk_kt + (size_t)i * G::KTN;
    if (lane == 0) kt_row[(nin + 15) >> 4] = kmax_seen;  // behind the last multiple of 16: the largest key
    constexpr int U = 4, M = 6, STEP = 4;  // (M = 8: 399 us, 6: 391, 4: 405 -- two instructions per member read and key)
    // A read past the end of the own bucket meets keys of later buckets, which are larger (the bucket function is monotone)
    // and so count neither as smaller nor as equal: no bounds test per member.  Past the last candidate it meets +inf.
    // Past the last candidate: eight entries of +inf, so that the first M members are read at constant offsets from the
    // bucket's start with no clamp (three vector instructions per member less: k_knn_rank 407 -> 391 us)
    const int lim = nin;  // <= NMAX
    if (lane < 8) L.s.skey[nin + lane] = __builtin_inff();
    wave_sync();
#pragma unroll
    for (int g0 = 0; g0 < NG; g0 += U) {
        if (g0 * 64 >= nin) break;  // wave-uniform
        int s0[U], s1[U], less[U], eq[U], longest = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int b = ci[g0 + u] >> 16;
            s0[u] = b ? (int)cur16[b - 1] : 0;
            s1[u] = (g0 + u) * 64 + lane < nin ? (int)cur16[b] : s0[u];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float mk[M];
            static_assert(M <= 8, "end markers");
#pragma unroll
            for (int k = 0; k < M; k++) mk[k] = L.s.skey[s0[u] + k];  // s0 < nin: at most nin + 6
            less[u] = s0[u];
            eq[u] = 0;
            longest = max(longest, s1[u] - s0[u]);
#pragma unroll
            for (int k = 0; k < M; k++) {
                less[u] += mk[k] < key[g0 + u] ? 1 : 0;
                eq[u] += mk[k] == key[g0 + u] ? 1 : 0;
            }
        }
        longest = wave_max(longest);
        if (GD_DIAG_IS(d.rk_dbg, 7)) longest = 0;
#ifdef GD_DIAG
        if (lane == 0 && d.rk_dbg == 9) atomicMax(&d.rk_hist[514], longest);  // diagnostic: the most crowded bucket of this selection
#endif
        for (int j = M; j < longest; j += STEP) {
            float mkk[U][STEP];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < STEP; k++) mkk[u][k] = L.s.skey[min(s0[u] + j + k, lim)];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int k = 0; k < STEP; k++) {
                    less[u] += mkk[u][k] < key[g0 + u] ? 1 : 0;
                    eq[u] += mkk[u][k] == key[g0 + u] ? 1 : 0;
                }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool on = (g0 + u) * 64 + lane < nin;
            eqmask |= ((eq[u] > 1) & on) ? 1u << (g0 + u) : 0u;  // (a candidate meets itself once)
            ci[g0 + u] = (ci[g0 + u] & 0xffff) | ((less[u] + 1) << (16 + G::RSH));  // e = (less + 1) << RSH | tie, in bits 16..31
            // the key table for k_knn_finish: this key sits at the sorted slots [less, less + eq); whoever holds slot 16 j
            // writes entry j (candidates with equal keys write the same value)
            const int j = (less[u] + 15) >> 4;
            if (on && (j << 4) < less[u] + eq[u]) kt_row[j] = key[g0 + u];
        }
    }
    int too_many_ties = 0;
    const bool has_tie = __ballot(eqmask != 0u) != 0ull;  // the replay then compares ranks without their tie field
    if (has_tie) {
        // place among the candidates with the same key: those of them that come earlier in road order.  A rolled loop (the
        // register arrays are picked apart with selects on the wave-uniform g): twenty copies of it cost the common path
        // its registers
#pragma clang loop unroll(disable)
        for (int g = 0; g * 64 < nin; g++) {
            if (__ballot((eqmask >> g) & 1u) == 0ull) continue;  // wave-uniform
            int cg = 0;
#pragma unroll
            for (int k = 0; k < NG; k++) cg = k == g ? ci[k] : cg;
            int tie = 0;
            if ((eqmask >> g) & 1u) {
                // (the candidate's bucket made way for its rank: found again as the bucket whose range of sorted slots holds
                // `less`, eleven probes of the cursors -- this pass is rare)
                const int less_g = (int)((unsigned int)cg >> (16 + G::RSH)) - 1, p = g * 64 + lane;
                int lo = 0, hi = NB - 1;
#pragma clang loop unroll(disable)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((int)cur16[mid] > less_g) hi = mid; else lo = mid + 1;
                }
                const int b = lo;
                const int first = b ? (int)cur16[b - 1] : 0, end = (int)cur16[b];
                float kg = 0.f;  // the candidate's key, from its own entry of the bucket (the key registers are long gone)
                for (int m = first; m < end; m++) kg = (int)L.s.spos[m] == p ? L.s.skey[m] : kg;
                for (int m = first; m < end; m++) tie += (L.s.skey[m] == kg ? 1 : 0) & ((int)L.s.spos[m] < p ? 1 : 0);
            }
            too_many_ties |= tie > (int)TM ? 1 : 0;
#pragma unroll
            for (int k = 0; k < NG; k++) ci[k] |= k == g ? (tie & (int)TM) << 16 : 0;
        }
    }
    wave_sync();  // every read of the sorted arrays is done: their space becomes the slot -> road table
    GD_PHASE(5);
    if (GD_DIAG_IS(d.rk_dbg, 5)) return;
    if (__ballot(too_many_ties != 0) != 0ull) {
        if (lane == 0) {
            d.rk_n[i] = 0;
            d.rk_ticket[i] = ticket | RK_TIES;  // more than 32 candidates with one key (the place in the order stays taken)
            d.rk_fallback[group] = 1;
        }
        return;
    }
    // (rows through scalar base addresses and unsigned 32-bit lane offsets: see `uni` above)
    // The slot -> road table goes on for its first SPL slots only: the K elements the replayed heap ends with are the K
    // smallest keys (slot < K + 31 with equal keys), and that is all k_knn_finish looks up by slot -- the checkpoints'
    // K-th keys come from the key table above (round 3 wrote all CAP slots, 2.5 KB per agent, and k_knn_finish fetched the
    // whole row back for 240 scattered 2-byte reads)
    unsigned short *const E_row = G::LONG ? d.rk_E_long + (size_t)uni(in.li) * CAP_LONG : d.rk_E + (size_t)i * CAP;
    const unsigned int ulane = (unsigned int)lane;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        if (g * 64 < nin) {  // wave-uniform
            if (g * 64 + lane < nin) {
                const unsigned int e = (unsigned int)ci[g] >> 16;
                stream_store((unsigned short)e, E_row + (g * 64u + ulane));
                const int slot = (int)(e >> G::RSH) - 1 + (int)(e & TM);
                if (slot < SPL) L.spc[slot] = (unsigned short)(ci[g] & 0xffff);
            }
        }
    }
    wave_sync();
    {
        static_assert(SPL == 256, "four slots per lane");
        const uint2 v = reinterpret_cast<const uint2 *>(L.spc)[lane];
        stream_store(v, reinterpret_cast<uint2 *>(d.rk_spc + (size_t)i * SPL) + ulane);
    }
    if (lane == 0) {
        d.rk_n[i] = nin | (nle << 16) | (has_tie ? 1 << 28 : 0) | (G::LONG ? 1 << 29 : 0);
        if (G::LONG) d.rk_longslot[i] = uni(in.li);
        d.rk_ticket[i] = ticket;
    }
    GD_PHASE(6);
}

// A wave ranks several agents in turn: tens of thousands of one-agent workgroups cost more in workgroup launches (each is
// handed its LDS first) than in work.
template <int A_T, int CAP_T>
__global__ __launch_bounds__(64, CAP_T > CAP ? 2 : 4) void k_knn_rank(DevSim d) {
    // (standard: at most 128 registers, four waves per SIMD like the LDS.  Measured: three waves per SIMD without spills
    // 437 us, four with seven spilled registers 391.  Long lists: 20 KB of LDS, two waves per SIMD, twice the registers)
    if (d.gate_any && *d.any_reset == 0) return;
    __shared__ RankLds<CAP_T> L;
    // Which agents a wave takes.  Standard: workgroup b runs on XCD b % 8 and shares out the list of the agents that
    // k_knn_scan's workgroups on that XCD put on the rank path (rk_list): a wave draws one entry per turn from the list's
    // cursor (rk_hist[GD_RH_CURSOR ..], zero when the launch starts: k_knn_order of the selection before, the rebuild) until
    // the draw is at or beyond the list's end.  An agent's cost varies (candidates 351 .. 854 beyond K on the bench scene,
    // and the same agent slot of the same scene costs the same step after step), and a fixed share of entries t, t + stride, ..
    // gave every wave eight turns of ONE agent slot: the launch lasted as long as the wave with the dearest slot.  Drawn, a
    // wave that got cheap agents takes more of them.  The entry for turn n + 1 is drawn at the start of turn n, so its
    // answer is back long before rank_fetch asks for that agent.  No wave takes from another XCD's list.  The road points an
    // agent gathers (32 KB per world on the bench scene) are then in that XCD's L2 already, and the waves resident at a time
    // work on a few dozen worlds instead of all of them (in agent-major order every generation of waves touched every world:
    // 32 MB against 4 MB of L2 per XCD; HBM bytes of the road observation 2.16 -> 1.36 GB per step).  Long lists: the one
    // list that the standard launch made of the agents it could not hold, entries b, b + gridDim.x, .. for wave b.
    // The cursors are asked only where there is something to share out: thousands of waves adding to one address cost tens
    // of microseconds.  (Measured with the long list on a cursor of its own: 2048 waves from every XCD on one address, 21 us
    // with the list EMPTY, as it is in most selections; drawn behind a first turn by index, the unreduced Waymo tiles' step
    // still went from 0.953 to 0.978 ms.  So the long list keeps its fixed shares.)  A standard list that has a turn for each
    // wave at most is shared out by index too (the deal it always had; nothing to balance there, and on the Waymo tiles every
    // wave asking once cost more than the kernel gained); otherwise every turn is drawn -- only half of the standard launch's
    // waves are resident at a time, and entries kept for the others would wait for the first wave to leave.  A wave with
    // nothing to take leaves before it asks.
    constexpr bool LONG = RankGeo<CAP_T>::LONG;
    const int xcd = blockIdx.x & 7;  // (the standard grid is a multiple of 8 workgroups)
    const int count = LONG ? min(uniform_load(d.rk_hist + GD_RH_LONG), d.rk_nlong) : uniform_load(d.rk_hist + 528 + xcd);
    const int *list = LONG ? d.rk_longlist : d.rk_list + (size_t)xcd * d.W * A_T;
    int *const cursor = d.rk_hist + GD_RH_CURSOR + xcd * GD_RH_CURSOR_STRIDE;
    const int share = LONG ? (int)gridDim.x : (int)(gridDim.x >> 3), mine = LONG ? (int)blockIdx.x : (int)(blockIdx.x >> 3);
    const bool fixed = LONG || count <= share;  // shares by index, no cursor
#ifdef GD_WAVE_CLOCKS
    // per wave of the standard launch: the constant 100 MHz clock at its start and at its end, the agents it ranked
    // (engine.hpp GD_RH_WAVES; tools/rank_waves.py takes the ends from the earliest start of the launch on the wave's XCD)
    int turns = 0;
    if (!LONG && threadIdx.x == 0) {
        const int now = (int)__builtin_amdgcn_s_memrealtime();
        d.rk_hist[GD_RH_WAVES + blockIdx.x] = now;
        d.rk_hist[GD_RH_WAVES + GD_RANK_GRID + blockIdx.x] = now;  // (a wave that leaves at once: no time, no agents)
        d.rk_hist[GD_RH_WAVES + 2 * GD_RANK_GRID + blockIdx.x] = 0;
    }
#endif
    if (fixed && mine >= count) return;
    // A drawn list is emptied by the waves the device holds at a time (d.rk_resident per list: the occupancy of this kernel, asked
    // when the simulator was created).  The launch has a wave per live agent, twice as many at 1024 x 64: those behind the
    // resident ones used to start when the first left, ask the cursor once each and find the list drawn empty.
    if (!fixed && mine >= d.rk_resident) return;
    int t = fixed ? mine : __builtin_amdgcn_readfirstlane(rank_draw(cursor, threadIdx.x));
    RankIn cur = rank_fetch<A_T>(d, list, t, count, threadIdx.x);
    PhaseClock clk;
#ifdef GD_CLOCKS
    for (int k = 0; k < 8; k++) clk.sum[k] = 0u;
    clk.prev = (unsigned int)__builtin_amdgcn_s_memtime();
#endif
    while (t < count) {
        RankIn nxt;
        GD_PHASE(0);  // between agents: the buffers change hands
        // (an opaque copy of the lane, per agent: what the ranking derives from the lane alone -- LDS addresses, row pointers,
        // positions -- is then computed per agent.  Hoisted out of this loop those values sat in registers, or in scratch,
        // through every phase, and the kernel has no register to spare)
        int lane_v = threadIdx.x;
        asm volatile("" : "+v"(lane_v));
        const int drawn = fixed ? t + share : rank_draw(cursor, lane_v);  // the turn after this one
        rank_agent<A_T, CAP_T>(d, cur, lane_v, L, clk, drawn, count, list, nxt);
        wave_sync();  // the LDS buffers change hands
        cur = nxt;
        t = __builtin_amdgcn_readfirstlane(nxt.li);
#ifdef GD_WAVE_CLOCKS
        turns++;
#endif
    }
#ifdef GD_CLOCKS
    if (threadIdx.x == 0)
        for (int k = 0; k < 8; k++) atomicAdd(reinterpret_cast<unsigned int *>(&d.rk_hist[516 + k]), clk.sum[k] >> 8);
#endif
#ifdef GD_WAVE_CLOCKS
    if (!LONG && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last agent's stores are part of the wave's time
        d.rk_hist[GD_RH_WAVES + GD_RANK_GRID + blockIdx.x] = (int)__builtin_amdgcn_s_memrealtime();
        d.rk_hist[GD_RH_WAVES + 2 * GD_RANK_GRID + blockIdx.x] = turns;
    }
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// k_knn_replay
// ------------------------------------------------------------------------------------------------------------------
// The heap of lane `l`: slots 1..K (1-based; the reference's array index is slot - 1) as u16 ranks, two per dword:
// pair j = (slot 2j, slot 2j + 1) at s_pair[j * 64 + l], so the children of slot g are pair g.  Slot K + 1 and, during
// the replay, slot K (whose element lives in a register) hold 0, which is below every rank.
#ifndef GD_RANK_AWR
#define GD_RANK_AWR 64
#endif
// agents per wave of the replay.  The round is one dependent chain (about 140 instructions and four LDS round trips), so a
// wave is as fast alone on its SIMD as beside a second one; measured at 1024 x 64 (us): 64 per wave 458, 32 per wave (two
// waves per SIMD) 492, 16 per wave 674; Waymo tiles 245 / 256 / 261 (tools/build_expt.sh awr32 -DGD_RANK_AWR=32)
constexpr int AWR = GD_RANK_AWR;
// (the same bytes are read and written as dwords and as halves: both types may alias, or the compiler is free to move a pair's
// load over the store of one of its halves -- with make_heap's straight-line groups it did)
typedef unsigned int __attribute__((may_alias)) heap_u32;
typedef unsigned short __attribute__((may_alias)) heap_u16;
struct RankHeap {
    heap_u32 *pr;  // this lane's column
    __device__ __forceinline__ unsigned int pair(int j) const { return pr[j * AWR]; }
    __device__ __forceinline__ unsigned int get(int g) const {
        return reinterpret_cast<const heap_u16 *>(pr + (g >> 1) * AWR)[g & 1];
    }
    __device__ __forceinline__ void set(int g, unsigned int v) const {
        reinterpret_cast<heap_u16 *>(pr + (g >> 1) * AWR)[g & 1] = (unsigned short)v;
    }
    __device__ __forceinline__ void set_pair(int j, unsigned int v) const { pr[j * AWR] = v; }
};
static_assert(rank_heap::NPAIR == 128, "s_pair of k_knn_replay");

// Replay order: the agents on the rank path sorted by candidate count, longest first (counting sort over 256 bins: k_knn_rank
// takes a ticket in its bin, every workgroup of this kernel turns the bin counts into starts for itself -- 256 loads and a
// scan, cheaper than the kernel boundary that a launch of its own for them cost -- and places its agents).  A wave's rounds
// are its longest agent's, so agents of similar length share a wave; which wave an agent rides never changes its result.
// The bin counts stay as they are until k_knn_replay's first workgroup zeroes them for the next selection: every
// workgroup here reads them.
__global__ __launch_bounds__(256) void k_knn_order(DevSim d) {
    if (d.gate_any && *d.any_reset == 0) return;
    __shared__ int s_part[4];
    __shared__ int s_start[256];
    const int tl = threadIdx.x;
    const int c = d.rk_hist[tl];
    const int incl = wave_incl_scan(c);
    if ((tl & 63) == 63) s_part[tl >> 6] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < (tl >> 6); k++) before += s_part[k];
    s_start[tl] = before + incl - c;  // start of bin tl
    if (blockIdx.x == 0 && tl == 255) {
        d.rk_hist[512] = before + incl;  // agents on the rank path
        d.rk_hist[513]++;                // selections so far (k_knn_scan staggers the retries of bypassing groups with it)
        for (int x = 0; x < 8; x++) d.rk_hist[528 + x] = 0;  // the next selection's lists of ranked agents start empty
        d.rk_hist[GD_RH_LONG] = 0;
        for (int x = 0; x < 8; x++) d.rk_hist[GD_RH_CURSOR + x * GD_RH_CURSOR_STRIDE] = 0;  // ... and k_knn_rank draws them from the head
    }
#ifdef GD_CLOCKS
    if (blockIdx.x == 0) d.rk_hist[256 + tl] = 0;  // k_knn_replay's phase clocks of this selection
#endif
    __syncthreads();
    const int t = blockIdx.x * 256 + tl;
    if (t >= d.live_count) return;
    const int i = d.live_list[t];
    const int ticket = d.rk_ticket[i];
    {
        // rows k_knn_scan wrote for ranked agents (gd_stat 22): none in a selection where every agent kept its own bound, so no
        // wave adds then (k_knn_scan zeroed the count; a thousand workgroups adding to one address cost it 10 us)
        const unsigned long long rows = __ballot(ticket >= 0 && (__float_as_int(d.rk_rec[i].z) & GD_RK_REC_ROW) != 0);
        if (rows != 0ull && (tl & 63) == 0) atomicAdd(&d.rk_hist[GD_RH_ROWS], __popcll(rows));
    }
    if (ticket < 0) return;  // not on the rank path
    d.rk_order[audited(d, s_start[(ticket >> 20) & 255] + (ticket & 0xfffff), d.W * d.A)] = i;
}

#ifdef GD_CLOCKS
// -DGD_CLOCKS: ticks of the constant 100 MHz clock (s_memrealtime; s_memtime counts shader cycles, whose rate moves) per phase of
// a replay wave -- 0 set-up (order, candidate count), 1 fill, 2 make_heap, 3 the rounds, 4 the heap's write-out -- kept per
// launch in rk_hist[256..]: seven values (the phases; bit 0: the wave ran the copy for equal keys, bits 1..9: its blocks in
// the equal-key form, bits 10..19: in the checked form, bits 20..: its blocks; the total) for each of the first 32 waves,
// which hold the longest agents; [480] waves on the equal-key copy, [481] waves that ran, [482] the longest total of any wave,
// [483] of any wave on the equal-key copy, [484] of any other wave; over the launch [485] blocks in the equal-key form, [486]
// blocks of the waves on the equal-key copy, [487] blocks in the checked form, [488] inserts (lanes) in rounds of the checked
// form, [489] those of them redone in the equal-key form.  k_knn_order zeroes them;
// gd_stat 1000 + k reads rk_hist[256 + k] (tools/replay_clocks.py).
struct ReplayClock {
    unsigned int prev, first, ph[5];
    __device__ __forceinline__ void start() { first = prev = (unsigned int)__builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void mark(int n) {
        const unsigned int t = (unsigned int)__builtin_amdgcn_s_memrealtime();
        ph[n] = t - prev;
        prev = t;
    }
};
#define GD_RPHASE(n) rclk.mark(n)
#else
#define GD_RPHASE(n)
#endif
__global__ __launch_bounds__(64) void k_knn_replay(DevSim d) {
    if (d.gate_any && *d.any_reset == 0) return;
    const int lane = threadIdx.x;
#ifdef GD_CLOCKS
    ReplayClock rclk;
    rclk.start();
#endif
    if (blockIdx.x == 0)  // the bin counts of this selection have been read by every workgroup of k_knn_order: ready for the next
        for (int k = 0; k < 4; k++) d.rk_hist[k * 64 + lane] = 0;
    const int li = blockIdx.x * AWR + lane;
    constexpr int NPAIR = 128;  // pairs 0..K/2 hold the heap; K/2 + 1 .. 127 stay 0: the "children" of slots beyond the heap
    __shared__ unsigned int s_pair[NPAIR * AWR];
    const RankHeap H{reinterpret_cast<heap_u32 *>(s_pair) + (lane % AWR)};
    int i = 0, n = 0, has_tie = 0, is_long = 0;
    if (lane < AWR && li < d.rk_hist[512]) {
        i = d.rk_order[li];
        const int packed = d.rk_n[i];
        n = packed & 0xffff;
        has_tie = (packed >> 28) & 1;
        is_long = (packed >> 29) & 1;  // ranked by the long-list instantiation: its own rows, tile and rank format
        if (d.rk_fallback[i / 32] != 0) n = 0;  // the whole group is selected by k_map_obs
    }
    const bool on = n >= K;  // (with fewer than 64 agents per wave: never true for the upper lanes, which share LDS columns with the lower ones)
    if (__ballot(on) == 0ull) return;
    const unsigned short *E = (on && is_long) ? d.rk_E_long + (size_t)d.rk_longslot[i] * CAP_LONG : d.rk_E + (size_t)i * CAP;
    const unsigned int tm = is_long ? 15u : 31u;  // equal-key field of this agent's ranks (RankGeo::RSH)
    const int tsh = is_long ? 6 : 5;             // log2 (candidates between its checkpoints)

    // ---- the first K candidates are roads 0..K-1 in order (src/knn.hpp:112-120) ----
    // All 25 blocks of the agent's first K ranks are requested together and waited for once (one at a time they were 25 memory
    // round trips in series in front of every wave's first round; k_knn_rank wrote the rows with streaming stores, so most
    // of them come from HBM).  Every lane loads, idle ones too (they read a row that exists: their own or row 0).
    const bool wave_ties = __ballot(on && has_tie) != 0ull;
    rank_heap::TieTrack tt{rank_heap::NO_TIE};  // this lane's heap: elements with a non-zero tie field (rank_heap.hpp)
    GD_RPHASE(0);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(E);
        unsigned int w[K / 2];
#pragma unroll
        for (int k = 0; k < K / 8; k++) {
            const uint4 v = stream_load(src + k);
            w[k * 4 + 0] = v.x;
            w[k * 4 + 1] = v.y;
            w[k * 4 + 2] = v.z;
            w[k * 4 + 3] = v.w;
        }
        if (lane < AWR) rank_heap::fill_pairs<K>(H, w);  // whole pairs; pair 0's low half, slot K + 1 and pairs K/2 + 1 .. 127: 0
        // equal keys among the first K of some lane (rare even in a wave with equal keys: an OR over the registers tells)
        if (wave_ties && __ballot(on && rank_heap::any_tie(w, tm)) != 0ull) {
            tt = rank_heap::track_of(w, tm);
            if (!on) tt.tg = rank_heap::NO_TIE;
        }
    }
    const bool heap_ties = __ballot(tt.tl()) != 0ull;  // make_heap compares equal keys
    GD_RPHASE(1);
    // ---- make_heap, src/binary_heap.hpp:170-185: parents K/2 .. 1, each __adjust_heap(hole, len = K, value) ----
    // (rank_heap.hpp: the sifts of one tree level in groups of eight, straight-line, two levels per LDS round trip)
    if (on) {
        if (heap_ties) rank_heap::make_heap<K, true>(H, tm);
        else rank_heap::make_heap<K, false>(H, tm);
    }
    GD_RPHASE(2);
    unsigned int r[8];             // slots 1..7 (tree levels 0..2) live in registers during the replay; r[1] is heap[0]
#pragma unroll
    for (int j = 1; j < 8; j++) r[j] = H.get(j);
    unsigned int last = H.get(K);  // heap[K - 1], kept in a register as well
    unsigned int q[4];             // ... and slots 12, 25, 50, 100, the rest of slot K's ancestors (rank_heap.hpp: mirrors, the column keeps them too)
    rank_heap::load_chain(H, q);
    if (lane < AWR) H.set(K, 0u);
    unsigned short *cpe = d.rk_cpe + (size_t)i * NCP;
    if (on) cpe[0] = (unsigned short)r[1];

    // ---- roads K.. : pop_heap + replace last + push_heap per insert (src/knn.hpp:128-151) ----
    int nmax = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, __shfl_xor(nmax, off));
    const uint4 *blocks = reinterpret_cast<const uint4 *>(E + K);  // K * 2 bytes: 16-byte aligned
    uint4 cur = on ? (GD_NT_REPLAY_LOAD ? stream_load(blocks) : blocks[0]) : make_uint4(0u, 0u, 0u, 0u);
    uint4 nxt = on ? (GD_NT_REPLAY_LOAD ? stream_load(blocks + 1) : blocks[1]) : make_uint4(0u, 0u, 0u, 0u);
    // Two copies of the loop, each over rank_heap.hpp's rounds.  When none of the wave's agents has two candidates with one
    // key (k_knn_rank reports it), every rank's tie field is 0 and every block of eight rounds runs the plain form (integer
    // compares, max / med3 / min).  The other copy decides per block, wave-uniformly (rank_heap.hpp Form): the form for equal
    // keys (compare without the tie field, select; about 1.2 x the plain one) only where a candidate of the block has a
    // non-zero tie field -- the second and later members of a group of equal keys; the checked form -- plain rounds, each
    // redone in the equal-key form if it met a tied rank -- while some lane holds such an element in its heap (TieTrack);
    // the plain form otherwise.  One lane in 200 has such a group at all, but a wave that ran the equal-key form throughout
    // because of that lane was the kernel's last wave in every launch.
#ifdef GD_CLOCKS
    int n_ins = 0;  // inserts of this lane's agent (gd_stat 20: total over the agents; 19: their candidates beyond K; 18: rounds of the first wave)
    int blk_all = 0, blk_ties = 0, blk_checked = 0;  // blocks of this wave, those in the equal-key form, those in the checked form
    int n_chk = 0, n_redo = 0;                       // rounds of the checked form with an insert in this lane; those that met a tied rank
    const auto wave_any = [&](bool f) -> bool {
        const bool a = __ballot(f) != 0ull;
        n_chk++;
        n_redo += a ? 1 : 0;
        return a;
    };
#else
    const auto wave_any = [](bool f) -> bool { return __ballot(f) != 0ull; };  // over the lanes that insert in this round
#endif
    auto replay = [&](auto mixed_tag) {
        constexpr bool MIXED = decltype(mixed_tag)::value;
        // The ranks arrive eight at a time (16 bytes), two blocks ahead.  An outer loop per block: the request for block b + 2
        // is issued at the top and its registers are not touched for eight rounds (inside one flat loop the compiler copied the
        // freshly requested block into place at once, i.e. waited a memory round trip every eighth round: a quarter of the kernel)
        // A tile of 32 candidates (what lies between two checkpoints) is four blocks of eight, each block's rounds unrolled:
        // a round takes its rank out of the block's registers with one instruction, and the checkpoint is written once per
        // tile (round 3 shifted the block by 16 bits and tested for the checkpoint in every round: a dozen instructions of ~130)
        static_assert(TILE == 32, "four blocks of eight candidates per checkpoint");
#pragma clang loop unroll(disable)
        for (int p0 = K; p0 < nmax; p0 += TILE) {
#pragma clang loop unroll(disable)
            for (int pb = p0; pb < min(p0 + TILE, nmax); pb += 8) {
                const uint4 w8 = cur;
                cur = nxt;
                // may run past this agent's candidates: the array ends in slack.  Every lane, idle ones too (they read row 0):
                // a merge with the old value would wait for the data
                nxt = GD_NT_REPLAY_LOAD ? stream_load(blocks + ((pb - K) >> 3) + 2) : blocks[((pb - K) >> 3) + 2];
                const unsigned int wd[4] = {w8.x, w8.y, w8.z, w8.w};
                const int left = n - pb;  // candidates of this lane's agent from here on (idle lanes: n = 0)
                int ins;
                // (slack beyond n and idle lanes do not count: `left`, `on`; one block in seventy has such a candidate, so the
                // wave first asks whether any of the eight ranks of a lane has the field set, slack or not -- an OR of the
                // four words -- and sorts the ranks by `left` only if one has)
                if (MIXED && __ballot(on && rank_heap::any_tie(wd, tm)) != 0ull &&
                    __ballot(on && rank_heap::block_has_tie(wd, left, tm)) != 0ull) {
                    ins = rank_heap::block_rounds<K, rank_heap::TIES>(H, r, last, q, wd, left, tm, tt);
#ifdef GD_CLOCKS
                    blk_ties++;
#endif
                } else if (MIXED && __ballot(tt.tl()) != 0ull) {
                    ins = rank_heap::block_rounds<K, rank_heap::CHECKED>(H, r, last, q, wd, left, tm, tt, wave_any);
#ifdef GD_CLOCKS
                    blk_checked++;
#endif
                } else {
                    ins = rank_heap::block_rounds<K, rank_heap::PLAIN>(H, r, last, q, wd, left, tm, tt);
                }
#ifdef GD_CLOCKS
                n_ins += ins;
                blk_all++;
#else
                (void)ins;
#endif
            }
            // after candidate (p0 - K) + 32: a checkpoint of every standard agent, of a long list at every second tile
            const int after = p0 - K + TILE;
            if (p0 + TILE - 1 < n && (after & ((1 << tsh) - 1)) == 0) cpe[after >> tsh] = (unsigned short)r[1];
        }
    };
    if (wave_ties) replay(std::true_type{});
    else replay(std::false_type{});
    GD_RPHASE(3);
#ifdef GD_CLOCKS
    {
        const int tot_ins = wave_sum(n_ins), tot_cand = wave_sum(on ? n - K : 0), longest = wave_max(on ? n - K : 0);
        if (lane == 0) {
            atomicAdd(&d.rk_hist[526], tot_ins);
            atomicAdd(&d.rk_hist[525], tot_cand);
            if (blockIdx.x == 0) atomicAdd(&d.rk_hist[524], longest);  // rounds of the longest wave
        }
    }
#endif
    // ---- the heap array, slot order, for k_knn_finish ----
    if (lane < AWR) {
        H.set(K, last);
#pragma unroll
        for (int j = 1; j < 8; j++) H.set(j, r[j]);
    }
    if (on) {
        unsigned int *out = d.rk_heap + (size_t)i * GD_RANK_HEAP_DW;
#pragma clang loop unroll(disable)
        for (int j = 0; j < GD_RANK_HEAP_DW; j += 4) {
            uint4 v;
            v.x = j + 0 <= K / 2 ? H.pair(j + 0) : 0u;
            v.y = j + 1 <= K / 2 ? H.pair(j + 1) : 0u;
            v.z = j + 2 <= K / 2 ? H.pair(j + 2) : 0u;
            v.w = j + 3 <= K / 2 ? H.pair(j + 3) : 0u;
            stream_store(v, reinterpret_cast<uint4 *>(out + j));
        }
    }
#ifdef GD_CLOCKS
    GD_RPHASE(4);
    const int w_chk = wave_sum(n_chk), w_redo = wave_sum(n_redo);
    if (lane == 0) {
        const int total = (int)(rclk.prev - rclk.first);
        if (blockIdx.x < 32) {
            int *row = d.rk_hist + 256 + blockIdx.x * 7;
            for (int k = 0; k < 5; k++) row[k] = (int)rclk.ph[k];
            row[5] = (wave_ties ? 1 : 0) | (blk_ties << 1) | (blk_checked << 10) | (blk_all << 20);  // (at most 2552 / 8 blocks)
            row[6] = total;
        }
        atomicAdd(&d.rk_hist[480], wave_ties ? 1 : 0);
        atomicAdd(&d.rk_hist[481], 1);
        atomicMax(&d.rk_hist[482], total);
        atomicMax(&d.rk_hist[wave_ties ? 483 : 484], total);
        atomicAdd(&d.rk_hist[485], blk_ties);
        atomicAdd(&d.rk_hist[486], wave_ties ? blk_all : 0);
        atomicAdd(&d.rk_hist[487], blk_checked);
        atomicAdd(&d.rk_hist[488], w_chk);
        atomicAdd(&d.rk_hist[489], w_redo);
    }
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// k_knn_finish: one wave per agent.  Heap array (ranks) -> road indices, radiusFilter, the checkpoints' K-th keys, and the
// hand-over to k_map_rows: the selected roads in ASCENDING road index with the output row each belongs in.
// Everything it reads is a contiguous piece of the agent's scratch rows: the heap (416 B), the first SPL sorted slots
// (512 B), the key table (336 B), the checkpoint ranks (80 B).
// ------------------------------------------------------------------------------------------------------------------
template <int A_T>
__global__ __launch_bounds__(256) void k_knn_finish(DevSim d) {
    if (d.gate_any && *d.any_reset == 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = blockIdx.x * 4 + wave;
    // the replay order: exactly the agents whose replay has run.  (The grid is sized for every live agent; the entry is
    // requested together with the count -- behind the count's end the array holds agent slots of earlier selections or zeros,
    // valid addresses all -- so that the wave's loads below are one round trip behind this one, not two)
    const int ranked_agents = d.rk_hist[512];
    const int i = d.rk_order[min(li, d.W * A_T - 1)];
    // Everything the wave reads from global memory depends on `i` alone and every address is valid for any agent slot (stale
    // at worst): requested together, before the first branch looks at any of it -- the kernel is a chain of memory round
    // trips with little arithmetic in between (round 3's version asked for flag, count, pose, heap and table one after the
    // other, each behind a branch on the one before)
    constexpr int NP = (K + 63) / 64;
    const int w = i / A_T;
    const int fell_back = d.rk_fallback[i / 32];
    const int packed = d.rk_n[i];
    const int r0 = d.road_off[w], r1 = d.road_off[w + 1];
    const float ex = d.px[i], ey = d.py[i];
    const float qw = d.qw[i], qz = d.qz[i];
    const uint32_t steps_left = d.steps[i];
    const int long_slot = d.rk_longslot[i];  // (meaningful only for an agent of the long-list instantiation: bit 29 of rk_n)
    const unsigned int *hp = d.rk_heap + (size_t)i * GD_RANK_HEAP_DW;
    unsigned int hpair[NP];
#pragma unroll
    for (int ps = 0; ps < NP; ps++) hpair[ps] = GD_NT_FINISH_LOAD ? stream_load(hp + min((ps * 64 + lane + 1) >> 1, GD_RANK_HEAP_DW - 1)) : hp[min((ps * 64 + lane + 1) >> 1, GD_RANK_HEAP_DW - 1)];
    static_assert(SPL == 256, "four slots per lane");
    const uint2 spc4 = GD_NT_FINISH_LOAD ? stream_load(reinterpret_cast<const uint2 *>(d.rk_spc + (size_t)i * SPL) + lane) : reinterpret_cast<const uint2 *>(d.rk_spc + (size_t)i * SPL)[lane];
    const unsigned int cp_e = d.rk_cpe[(size_t)i * NCP + min(lane, NCP - 1)];
    const unsigned short cp_r = d.cp_road[(size_t)i * NCP + min(lane, NCP - 1)];
    // (the compiler otherwise sinks each of these loads below the early returns that do not need it: flag, branch, count,
    // branch, the rest -- three round trips instead of one.  Naming them all as inputs here keeps them together above the
    // first branch)
    static_assert(NP == 4, "operand list");
    asm volatile("" ::"v"(fell_back), "v"(packed), "v"(ex), "v"(ey), "v"(qw), "v"(qz), "v"(steps_left), "v"(long_slot), "v"(hpair[0]),
                 "v"(hpair[1]), "v"(hpair[2]), "v"(hpair[3]), "v"(spc4.x), "v"(spc4.y), "v"(cp_e), "v"(cp_r), "s"(r0), "s"(r1));
    if (li >= ranked_agents || fell_back != 0) return;  // beyond the order / k_map_obs selects for this group
    // (agents out of reach of every road never get here: k_knn_scan wrote their empty hand-over)
    const int n = packed & 0xffff, nle = (packed >> 16) & 0xfff;
    if (packed <= 0 || packed == RK_FAR || n < K) return;  // took a place in the order, then fell back (equal keys)
    // the checkpoints' K-th keys (see below): the table entry is known as soon as the checkpoint's rank is
    const bool is_long = ((packed >> 29) & 1) != 0;
    const int rsh = is_long ? 4 : 5, tsh = is_long ? 6 : 5;  // rank format and checkpoint spacing (RankGeo)
    const unsigned int tm = (1u << rsh) - 1u;
    const int cp_slot = (int)(cp_e >> rsh) - 1 + (int)(cp_e & tm);
    const int ncp = 1 + ((n - K) >> tsh);
    const float *kt_row = is_long ? d.rk_kt_long + (size_t)long_slot * GD_RANK_KT_LONG : d.rk_kt + (size_t)i * KT;
    float cp_t = 0.f;
    if (lane < ncp) cp_t = kt_row[min(max((cp_slot + 15) >> 4, 0), (n + 15) >> 4)];
    __shared__ unsigned short s_spc[4][SPL];
    __shared__ unsigned short s_don[4][K];
    __shared__ unsigned int s_bm[4][GD_RANK_NCH];      // one bit per road of the world: selected
    __shared__ unsigned short s_wp[4][GD_RANK_NCH];    // selected roads below each bitmap word
    __shared__ unsigned int s_sorted[4][K];            // ascending road index -> road | output row << 16
    unsigned short *don = s_don[wave];
    unsigned int *bm = s_bm[wave];
    const unsigned long long lower = (1ull << lane) - 1ull;
    {
        reinterpret_cast<uint2 *>(s_spc[wave])[lane] = spc4;
#pragma unroll
        for (int k = 0; k < GD_RANK_NCH / 64; k++) bm[k * 64 + lane] = 0u;
    }
    wave_sync();

    // heap array -> road indices and in-radius flags (src/knn.hpp:88: length() <= radius; on ranks: fewer than `nle`
    // candidates have a smaller key)
    int road[NP];
    bool inr[NP];
    unsigned long long fl[NP];
    int m = 0;
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        const int t = ps * 64 + lane, g = t + 1;
        road[ps] = 0;
        inr[ps] = false;
        if (t < K) {
            const unsigned int p2 = hpair[ps];
            const unsigned int e = (g & 1) ? p2 >> 16 : p2 & 0xffffu;
            const int less = (int)(e >> rsh) - 1;
            // (a rank of 0 -- an element the replay never wrote -- would ask for slot -1; an element of the final heap has
            // fewer than K keys below it and at most 31 equal ones before it)
            road[ps] = s_spc[wave][audited(d, less + (int)(e & tm), min(n, SPL))];
            inr[ps] = less < nle;
        }
        fl[ps] = __ballot(inr[ps]);
        m += __popcll(fl[ps]);
    }
    // radiusFilter's swap-remove loop: with m in-radius elements, the out-of-radius slots below m (ascending) receive
    // the in-radius elements of [m, K) in DESCENDING slot order; everything else below m stays
    if (m < K) {
        int above = 0;  // in-radius slots above the current pass
#pragma unroll
        for (int ps = NP - 1; ps >= 0; ps--) {
            const int t = ps * 64 + lane;
            if (t < K && t >= m && inr[ps]) don[above + __popcll(fl[ps] & ~lower & ~(1ull << lane))] = (unsigned short)road[ps];
            above += __popcll(fl[ps]);
        }
        wave_sync();
        int before = 0;  // slots below the current pass
        int in_before = 0;
#pragma unroll
        for (int ps = 0; ps < NP; ps++) {
            const int t = ps * 64 + lane;
            if (t < m && !inr[ps]) {
                const int h = (t - before) - __popcll(fl[ps] & lower) + (before - in_before);  // out-of-radius slots below t
                road[ps] = don[h];
            }
            before += 64;
            in_before += __popcll(fl[ps]);
        }
    }
    // ---- hand-over: the m selected roads in ascending road index, each with its output row (k_map_rows gathers the
    // 32-byte records in that order and puts the rows where they belong).  A bitmap of the world's roads, prefix counts
    // per word, place = selected roads below. ----
    const int R = r1 - r0;
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        const int t = ps * 64 + lane;
        if (t < m) atomicOr(&bm[audited(d, road[ps], R) >> 5], 1u << (road[ps] & 31));
    }
    wave_sync();
    {
        constexpr int WL = GD_RANK_NCH / 64;  // bitmap words per lane: lane l owns words l * WL ..
        unsigned int own[WL];
        int sum = 0;
#pragma unroll
        for (int k = 0; k < WL; k++) { own[k] = bm[lane * WL + k]; sum += __popc(own[k]); }
        int run = wave_incl_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < WL; k++) { s_wp[wave][lane * WL + k] = (unsigned short)run; run += __popc(own[k]); }
    }
    wave_sync();
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        const int t = ps * 64 + lane;
        if (t < m) {
            const int rd = min(max(road[ps], 0), R - 1);
            const int place = (int)s_wp[wave][rd >> 5] + __popc(bm[rd >> 5] & ((1u << (rd & 31)) - 1u));
            s_sorted[wave][audited(d, place, m)] = (unsigned int)rd | (unsigned int)t << 16;
        }
    }
    wave_sync();
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        const int q = ps * 64 + lane;
        if (q < K) {
            const unsigned int v = q < m ? s_sorted[wave][q] : (unsigned int)q << 16;
            d.sel_idx[(size_t)i * K + q] = (unsigned short)(v & 0xffffu);
            d.sel_slot[(size_t)i * K + q] = (unsigned char)(v >> 16);
        }
    }
    // the K-th distances at this selection's checkpoints: a key that is not below that of the element whose rank was on top
    // -- from the key table, the candidates' key at the next multiple of 16 sorted slots (any upper bound of the K-th
    // distance keeps the next selection's candidates a superset; this one is at most 15 ranks loose)
    // (a second copy is kept of the selection made at the start of an episode: a reset puts the agent back there)
    const bool at_start = steps_left == (uint32_t)GD_EPISODE_LEN;
    const size_t WA = (size_t)d.W * A_T;
    if (lane < ncp) {
        (void)audited(d, cp_slot, n);  // (a rank of 0 on top of the heap at a checkpoint: never written by the replay)
        d.cp_T[(size_t)i * NCP + lane] = cp_t;
        if (at_start) {
            d.cp_T[(WA + i) * NCP + lane] = cp_t;
            d.cp_road[(WA + i) * NCP + lane] = cp_r;
        }
    }
    if (lane == 0) {
        d.rk_streak[i / 32] = 0;  // the group got through without the fallback
        d.cp_hdr[i] = make_float4(ex, ey, __int_as_float(ncp), 0.f);
        if (at_start) d.cp_hdr[WA + i] = make_float4(ex, ey, __int_as_float(ncp), 0.f);
        d.sel_hdr[(size_t)i * 2] = make_float4(ex, ey, qw, qz);
        d.sel_hdr[(size_t)i * 2 + 1] = make_float4(__int_as_float(m), __int_as_float(r0), __int_as_float(1), 0.f);
    }
}

}  // namespace

#ifndef GD_RANK_LONG_GRID
#define GD_RANK_LONG_GRID 2048  // (an empty launch costs 5 us whatever its size; 256 waves ranked the long lists of the unreduced Waymo tiles in 614 us, 2048 in 157)
#endif
int rank_resident_waves(int A) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    const hipError_t e = A == 64 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_knn_rank<64, CAP>, 64, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_knn_rank<128, CAP>, 64, 0);
    if (e != hipSuccess || hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        (void)hipGetLastError();
        return GD_RANK_GRID;  // nothing leaves early: the launch as it was
    }
    return std::max(per_cu, 1) * std::max(prop.multiProcessorCount, 1);
}

void launch_map_obs_rank(const DevSim &d, hipStream_t st) {
    if (d.live_count == 0) return;
    // the long-list ranking: persistent waves (eight per CU fit) over however many agents the standard launch passed on (none:
    // every wave reads the empty count and leaves)
    const dim3 glong(std::min(std::max(d.rk_nlong, 1), GD_RANK_LONG_GRID));
    const dim3 gr(d.rk_waves > 0 ? d.rk_waves : std::min((d.live_count + 7) / 8 * 8, GD_RANK_GRID)), g4((d.live_count + 3) / 4), gw(d.W * (d.A / 64));  // rank: 8192 persistent waves, 16 per CU resident (LDS)
    // the set-up: run by the state step of this pass (engine.hpp rank_setup_folded), or the launch of its own (GPUDRIVE_RANK_SCAN_KERNEL=1)
    const bool scan = !rank_setup_folded(d);
    if (d.A == 64) {
        if (scan) hipLaunchKernelGGL((k_knn_scan<64>), gw, dim3(256), 0, st, d);
        hipLaunchKernelGGL((k_knn_rank<64, CAP>), gr, dim3(64), 0, st, d);
        if (d.rk_nlong > 0) hipLaunchKernelGGL((k_knn_rank<64, CAP_LONG>), glong, dim3(64), 0, st, d);
    } else {
        if (scan) hipLaunchKernelGGL((k_knn_scan<128>), gw, dim3(256), 0, st, d);
        hipLaunchKernelGGL((k_knn_rank<128, CAP>), gr, dim3(64), 0, st, d);
        if (d.rk_nlong > 0) hipLaunchKernelGGL((k_knn_rank<128, CAP_LONG>), glong, dim3(64), 0, st, d);
    }
    hipLaunchKernelGGL(k_knn_order, dim3((d.live_count + 255) / 256), dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_knn_replay, dim3((d.live_count + AWR - 1) / AWR), dim3(64), 0, st, d);
    if (d.A == 64) hipLaunchKernelGGL((k_knn_finish<64>), g4, dim3(256), 0, st, d);
    else hipLaunchKernelGGL((k_knn_finish<128>), g4, dim3(256), 0, st, d);
}

}  // namespace gd
