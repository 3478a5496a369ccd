// The rank path's candidate set (map_obs_rank.hip k_knn_scan -> k_knn_rank) as plain C++: the decisions that the kernel and
// a host program share (tests/rank_cand_model.cpp runs the cull + in-order scan below against a plain loop over every road;
// tests/rank_cp_table_model.cpp the cull's table of checkpoints per chunk, (b') below, against the counts of (b);
// tests/rank_setup_model.cpp the row made of an agent's own checkpoints, (b''), and the deal of worlds to workgroups, (d)).
//
// An agent's candidates are roads 0..K-1 plus every later road r < R whose cheap squared distance is below the threshold of
// the CHECKPOINT in force for r.  k_knn_scan leaves a row of checkpoints per agent: first[q] (a multiple of 32) and thr[q];
// the checkpoint in force for a road is the last q with first[q] <= the base of the road's 32-road chunk, none (q = -1) means
// unbounded.  k_knn_rank finds the candidates in two steps:
//
//   cull  a lane per block of BLK consecutive roads (the circle the engine keeps around every such block, engine.hpp
//         road_blk): a block is dropped only if no road of it can pass the per-road test.  BLK divides 32 and first[] are
//         multiples of 32, so a block lies inside one checkpoint's range and is tested against one threshold.
//   scan  the surviving blocks in index order, every road of them through the per-road test.
//
// Why a dropped block holds no candidate.  Let D be the distance from the agent e to a road point p of the block, u = 2^-24.
// The per-road test computes dx = fl(x - ex) = (x - ex)(1 + d1), |d1| <= u, likewise dy, and d2 = fl(fma(dx, dx, fl(dy dy)))
// >= D^2 (1 - 4u); it passes only if d2 < thr, so D < sqrt(thr) (1 + 3u).  The block's circle (c, rad) holds p with the
// host's inflation (rad = computed radius * 1.0001 + 1e-3, engine.cpp: far above the rounding of its own arithmetic), so
// |c - e| <= D + rad, and the computed |c - e|^2 is at most (1 + 4u) times the true one.  The block test keeps the block
// unless  fl|c - e|^2 > (reach + rad)^2 * 1.00001  with  reach = fl(sqrt(thr)) * 1.00001 >= sqrt(thr) (1 + 9e-6): every factor
// of (1 + a few u) above is covered by the two factors of 1.00001, so a block with a passing road is kept.  thr = inf gives
// reach = inf and keeps every block; a NaN anywhere compares false and keeps the block.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define GD_RC_FN __host__ __device__ __forceinline__
#else
#define GD_RC_FN inline
#endif

namespace gd {
namespace rank_cand {

constexpr int CHUNK = 32;                     // roads per chunk: first[] are multiples of it
constexpr unsigned int NO_CP = 0xffffffffu;   // first[] of a row entry behind the agent's last checkpoint: never in force

GD_RC_FN unsigned int f32_bits(float f) { return __builtin_bit_cast(unsigned int, f); }

// (a) the per-road test, the expression and the sense of the scan it replaces: candidate <=> sign bit of d2 - thr
GD_RC_FN bool road_passes(float x, float y, float ex, float ey, float thr) {
    const float dx = x - ex, dy = y - ey;
    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
    return (f32_bits(d2 - thr) >> 31) != 0u;
}
// roads below K are candidates regardless, roads at or beyond R never
GD_RC_FN bool is_candidate(int r, int K, int R, float x, float y, float ex, float ey, float thr) {
    return r < R && (r < K || road_passes(x, y, ex, ey, thr));
}

// (b) the checkpoint in force for the roads of the chunk that starts at `base`: the scan's rule, q advances while the next
// entry starts at or before the chunk.  -1: none, the chunk is unbounded.
GD_RC_FN int cp_in_force(const unsigned int *first, int ncp, int base) {
    int q = -1;
    while (q + 1 < ncp && first[q + 1] <= (unsigned int)base) q++;
    return q;
}
// The same as a count: with first[] replaced by its running maximum (what k_knn_scan stores), the entries at or before the
// chunk are a prefix of the row, and its length is cp_in_force + 1 -- for ANY first[], non-decreasing or not.
GD_RC_FN unsigned int running_max(unsigned int run, unsigned int first) { return first > run ? first : run; }
GD_RC_FN int cp_count(const unsigned int *first_max, int n, int base) {
    int c = 0;
    for (int q = 0; q < n; q++) c += first_max[q] <= (unsigned int)base ? 1 : 0;
    return c;
}
GD_RC_FN int chunk_base_of_block(int b, int blk) { return (b * blk) & ~(CHUNK - 1); }

// (b'') a checkpoint's threshold: `t` is the K-th key a previous selection recorded at the checkpoint, `move` how far the agent
// is from where it was recorded (the K-th distance over a prefix of the roads is 1-Lipschitz in the position), `margin` covers
// rounding and the squared norm of the stored quaternion.  An unusable entry (NaN, a negative key) bounds nothing.  k_knn_scan
// (the rows it writes) and k_knn_rank (the rows it makes of the agent's own checkpoints) call this text, both built with
// -ffp-contract=off: the same bits.
GD_RC_FN float cp_threshold(float t, float move, float margin) {
    const float reach = sqrtf(t) * 1.0001f + move * 1.0001f + 1e-3f;
    const float thr = reach * reach * 1.0001f * margin;
    return thr >= 0.f ? thr : __builtin_inff();
}
constexpr float CP_MOVE_MAX = 6.f;  // beyond it an agent's own checkpoints are no use (k_knn_scan: a donor's, or bounded afresh)

// (d) which world a workgroup of k_knn_scan takes.  Workgroup b runs on XCD b % 8 and appends its agents to that XCD's list, so
// with the identity XCD x ranks the worlds x, x + 8, ..: when the scenes are tiled with a period that shares a factor with 8 (the
// bench's eight scenes, a loader that cycles through its files) one XCD gets every copy of the dearest scene and the ranking
// lasts as long as that XCD.  The deal rotates the eight blocks of every aligned group of 8 among themselves, group g by
// r(g) = g + g / 8 + g / 64 (mod 8): a bijection of [0, grid) that maps every aligned group onto itself -- a world still goes
// to ONE list -- and is the identity on a last partial group.
GD_RC_FN int deal_rotation(int g) { return (g + (g >> 3) + (g >> 6)) & 7; }
GD_RC_FN int deal_block(int b, int grid) {
    if ((b | 7) >= grid) return b;  // the last, partial group
    return (b & ~7) | ((b + deal_rotation(b >> 3)) & 7);
}
// The same deal from the world's side: the list (0..7) that world-block w belongs on, i.e. b % 8 of the b with deal_block(b) = w.
// k_knn_scan uses this form: workgroup w takes world-block w, on the XCD where the step's other kernels keep that world, and
// appends to list deal_list(w).
GD_RC_FN int deal_list(int w, int grid) {
    if ((w | 7) >= grid) return w & 7;
    return (w - deal_rotation(w >> 3)) & 7;
}

// (b') the same count for every chunk of a world at once, as a table that k_knn_rank builds once per agent: entry c is
// cp_count(first_max, n, c * CHUNK).  The row is non-decreasing, so the entries at or before a chunk are a prefix of it and their
// number is the largest q + 1 among them: checkpoint q leaves q + 1 in the entry of the first chunk it is in force for (SCATTER,
// a max where several checkpoints start in one chunk), and a running maximum over the chunks carries it to every later chunk
// (SCAN).  NO_CP and a first road behind the base of the world's last chunk are in force for no chunk of the world and leave
// nothing.  first[] are multiples of CHUNK in the engine; rounding up keeps the rule equal to cp_count for any value.
GD_RC_FN int chunks_of(int R) { return (R + CHUNK - 1) / CHUNK; }
GD_RC_FN unsigned int cp_table_chunk(unsigned int first_max) { return first_max / CHUNK + (first_max % CHUNK ? 1u : 0u); }
GD_RC_FN bool cp_table_takes(unsigned int first_max, int nchunks) {
    return first_max != NO_CP && cp_table_chunk(first_max) < (unsigned int)nchunks;
}
GD_RC_FN unsigned int cp_table_entry(int q) { return (unsigned int)q + 1u; }
// `tab`: nchunks entries.  (The kernel zeroes, scatters with an LDS max from lane q, and scans with each lane on consecutive entries.)
GD_RC_FN void cp_table(unsigned int *tab, int nchunks, const unsigned int *first_max, int n) {
    for (int c = 0; c < nchunks; c++) tab[c] = 0u;
    for (int q = 0; q < n; q++)
        if (cp_table_takes(first_max[q], nchunks)) {
            unsigned int &e = tab[cp_table_chunk(first_max[q])];
            e = cp_table_entry(q) > e ? cp_table_entry(q) : e;
        }
    for (int c = 1; c < nchunks; c++) tab[c] = tab[c - 1] > tab[c] ? tab[c - 1] : tab[c];
}

// (c) the block test.  `reach` is block_reach(thr of the checkpoint in force for the block), `rad` the host's inflated radius.
GD_RC_FN float block_reach(float thr) { return sqrtf(thr) * 1.00001f; }
GD_RC_FN bool block_survives(int b, int blk, int K, float cx, float cy, float rad, float ex, float ey, float reach) {
    const float dx = cx - ex, dy = cy - ey, rr = reach + rad;
    return b * blk < K || !(dx * dx + dy * dy > rr * rr * 1.00001f);  // a block with a road below K always survives
}

}  // namespace rank_cand
}  // namespace gd
