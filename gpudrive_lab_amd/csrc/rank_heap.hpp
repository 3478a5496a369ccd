// The prologue of the rank replay (map_obs_rank.hip k_knn_replay) as plain C++: the fill of the heap's first K slots and
// the reference's make_heap (src/binary_heap.hpp:170-185), written so that the device and a host program run the same code
// (tests/replay_heap_model.cpp holds it against std::make_heap).
//
// The heap: slots 1..K (1-based; the reference's array index is slot - 1) of 16-bit ranks, two per dword: pair j = (slot 2j,
// slot 2j + 1), so the children of slot g are pair g.  The low half of pair 0, slot K + 1 and the pairs K/2 + 1 .. NPAIR - 1
// hold 0, which is below every rank: the "children" of slots beyond the heap lose every comparison.
//
// A heap accessor `H` has  pair(j) -> dword,  get(slot) -> rank,  set(slot, rank),  set_pair(j, dword).
//
// make_heap is parents K/2 .. 1, each __adjust_heap(hole = g, len = K, value = x): the hole goes to the bottom along the larger
// child (the right one unless it is smaller), then x climbs back towards g past every moved child that is smaller.  The
// subtrees below g are heaps already, so the moved children ck[0..D-1] are non-increasing down the path, "x passes level l" is
// monotone in l, and the value that ends on level l is max(ck[0], x), then the median of (ck[l-1], ck[l], x), then
// min(ck[D-1], x): no climbing loop (the replay's pop does the same for its last element).  Sifts of parents on one tree level
// touch disjoint subtrees, so they commute: they run in groups of up to eight whose LDS reads are issued together, two levels
// per round trip, instead of one parent and one level at a time.  Levels run bottom-up, like the reference's descending g.
#pragma once

#if defined(__HIPCC__)
#define GD_RH_FN __host__ __device__ __forceinline__
#else
#define GD_RH_FN inline
#endif
#if defined(__clang__)
#define GD_RH_UNROLL _Pragma("unroll")
#define GD_RH_NO_UNROLL _Pragma("clang loop unroll(disable)")
#else
#define GD_RH_UNROLL
#define GD_RH_NO_UNROLL
#endif

namespace gd {
namespace rank_heap {

constexpr int NPAIR = 128;  // dwords of a heap column

GD_RH_FN unsigned int umax(unsigned int a, unsigned int b) { return a > b ? a : b; }
GD_RH_FN unsigned int umin(unsigned int a, unsigned int b) { return a < b ? a : b; }
GD_RH_FN unsigned int med3(unsigned int a, unsigned int b, unsigned int c) { return umax(umin(a, b), umin(umax(a, b), c)); }
// key comparison on ranks (map_obs_rank.hip rank_lt): the low bits under `tm` count the equal keys before a candidate
GD_RH_FN bool key_lt(unsigned int a, unsigned int b, unsigned int tm) { return (a | tm) < b; }

// The first K candidates are roads 0..K-1 in order: slot s holds E[s - 1].  `w` are the K/2 dwords of E[0..K-1], so pair j is
// the high half of w[j-1] under the low half of w[j]: whole pairs, one 32-bit store each.
template <int K, class Heap>
GD_RH_FN void fill_pairs(const Heap &H, const unsigned int (&w)[K / 2]) {
    static_assert(K % 2 == 0 && K / 2 < NPAIR, "pairs of a heap column");
    H.set_pair(0, w[0] << 16);
    GD_RH_UNROLL
    for (int j = 1; j < K / 2; j++) H.set_pair(j, (w[j] << 16) | (w[j - 1] >> 16));
    H.set_pair(K / 2, w[K / 2 - 1] >> 16);
    GD_RH_UNROLL
    for (int j = K / 2 + 1; j < NPAIR; j++) H.set_pair(j, 0u);
}

// Parents gt, gt - 1, .. gt - G + 1, all on one tree level with D levels below it (the last of them partly beyond slot K).
// TIES = false: none of the ranks has two candidates with one key, every tie field is 0, and an integer compare is the key compare.
template <int K, int G, int D, bool TIES, class Heap>
GD_RH_FN void sift_group(const Heap &H, const int gt, const unsigned int tm) {
    auto lt = [&](unsigned int a, unsigned int b) -> bool { return TIES ? key_lt(a, b, tm) : a < b; };
    auto larger = [&](unsigned int p2, bool &right) -> unsigned int {
        const unsigned int kl = p2 & 0xffffu, kr = p2 >> 16;
        right = !lt(kr, kl);
        return TIES ? (right ? kr : kl) : umax(kl, kr);
    };
    unsigned int x[G], ck[G][D];
    int g[G][D + 1];
    {  // levels 0 and 1: the addresses are the same for every heap
        unsigned int pc[G], pl[G], pr[G];
        GD_RH_UNROLL
        for (int m = 0; m < G; m++) {
            g[m][0] = gt - m;
            x[m] = H.get(g[m][0]);
            pc[m] = H.pair(g[m][0]);
            if constexpr (D >= 2) {
                pl[m] = H.pair(2 * g[m][0]);
                pr[m] = H.pair(2 * g[m][0] + 1);
            }
        }
        GD_RH_UNROLL
        for (int m = 0; m < G; m++) {
            bool ra, rb;
            ck[m][0] = larger(pc[m], ra);
            g[m][1] = 2 * g[m][0] + (ra ? 1 : 0);
            if constexpr (D >= 2) {
                ck[m][1] = larger(ra ? pr[m] : pl[m], rb);
                g[m][2] = 2 * g[m][1] + (rb ? 1 : 0);
            }
        }
    }
    GD_RH_UNROLL
    for (int l = 2; l < D; l += 2) {  // two more levels per round trip: a node's children pair and both grandchildren pairs
        unsigned int pc[G], pl[G], pr[G];
        GD_RH_UNROLL
        for (int m = 0; m < G; m++) {
            pc[m] = H.pair(g[m][l]);
            if (l + 1 < D) {
                pl[m] = H.pair(2 * g[m][l]);
                pr[m] = H.pair(2 * g[m][l] + 1);
            }
        }
        GD_RH_UNROLL
        for (int m = 0; m < G; m++) {
            bool ra, rb;
            ck[m][l] = larger(pc[m], ra);
            g[m][l + 1] = 2 * g[m][l] + (ra ? 1 : 0);
            if (l + 1 < D) {
                ck[m][l + 1] = larger(ra ? pr[m] : pl[m], rb);
                g[m][l + 2] = 2 * g[m][l + 1] + (rb ? 1 : 0);
            }
        }
    }
    GD_RH_UNROLL
    for (int m = 0; m < G; m++) {
        unsigned int v[D + 1];
        if (TIES) {
            bool c[D];
            GD_RH_UNROLL
            for (int l = 0; l < D; l++) c[l] = lt(ck[m][l], x[m]);
            GD_RH_UNROLL
            for (int l = 0; l <= D; l++) {
                if (l == 0) v[l] = c[0] ? x[m] : ck[m][0];
                else if (l == D) v[l] = c[D - 1] ? ck[m][D - 1] : x[m];
                else v[l] = c[l - 1] ? ck[m][l - 1] : (c[l] ? x[m] : ck[m][l]);
            }
        } else {
            v[0] = umax(ck[m][0], x[m]);
            GD_RH_UNROLL
            for (int l = 1; l < D; l++) v[l] = med3(ck[m][l - 1], ck[m][l], x[m]);
            v[D] = umin(ck[m][D - 1], x[m]);
        }
        GD_RH_UNROLL
        for (int l = 0; l <= D; l++)
            if (l < D || g[m][D] <= K) H.set(g[m][l], v[l]);  // only the last level reaches beyond the heap
    }
}

template <int K, bool TIES, class Heap>
GD_RH_FN void make_heap(const Heap &H, const unsigned int tm) {
    static_assert(K == 200, "tree levels of the parents: 64..100, 32..63, 16..31, 8..15, 4..7, 2..3, 1");
    GD_RH_NO_UNROLL
    for (int gt = 100; gt >= 76; gt -= 8) sift_group<K, 8, 1, TIES>(H, gt, tm);  // 100 .. 69
    sift_group<K, 5, 1, TIES>(H, 68, tm);                                          // 68 .. 64
    GD_RH_NO_UNROLL
    for (int gt = 63; gt >= 39; gt -= 8) sift_group<K, 8, 2, TIES>(H, gt, tm);
    GD_RH_NO_UNROLL
    for (int gt = 31; gt >= 23; gt -= 8) sift_group<K, 8, 3, TIES>(H, gt, tm);
    sift_group<K, 8, 4, TIES>(H, 15, tm);
    sift_group<K, 4, 5, TIES>(H, 7, tm);
    sift_group<K, 2, 6, TIES>(H, 3, tm);
    sift_group<K, 1, 7, TIES>(H, 1, tm);
}

}  // namespace rank_heap
}  // namespace gd
