// The rank replay (map_obs_rank.hip k_knn_replay) as plain C++: the fill of the heap's first K slots, the reference's
// make_heap (src/binary_heap.hpp:170-185) and the rounds (pop_heap, replace last, push_heap per insert, with the choice of
// the form that equal keys need), written so that the device and a host program run the same code
// (tests/replay_heap_model.cpp holds the prologue against std::make_heap, tests/replay_rounds_model.cpp the rounds against
// the reference algorithm on keys).
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

// ---- the rounds: one insert per candidate that passes the reference's test `cmp(current, heap[0])` (src/knn.hpp:138-143) ----
// During the rounds slots 1..7 (tree levels 0..2) live in `r[1..7]` (r[1] is heap[0]) and slot K in `last`; slot K's place in
// the column holds 0.  `q[0..3]` mirror slots 12, 25, 50, 100 -- with 1, 3, 6 the ancestors of slot K, the chain every push
// climbs.  Those slots are fixed and change only where the round has the new value in a register already (the pop, when its path
// goes through one of them, and the push's own store), so the round reads none of them back.  The column stays authoritative:
// every store of the pop and of the push is made as before (the pop reads these slots as halves of pairs), `q` only follows.
//
// One insert of candidate rank y: pop_heap, replace last, push_heap.
// pop_heap: the hole goes from the root to the bottom of the (K - 1)-element heap along the larger child.  Levels 0 and 1 are
// decided in registers; below that three, then two levels per LDS round trip: a node's children pair, its grandchildren pairs
// (and great-grandchildren pairs) are fetched together (pairs beyond the heap hold 0, which loses every comparison).  The
// ancestors of slot K that the push will meet come from `q`, patched where the pop's path went through them.  Where the path
// went is known from the choices made on the way down (slot 6 is the right-left grandchild of the root, 12 the left child of 6,
// 25 the right child of 12, 50 the left child of 25, 100 the left child of 50): lane masks that exist already, no compare of
// a slot number.
// TIES = false: a plain integer compare IS the key compare, "the larger child" is a max and the values along the pop's path
// and the push's chain are medians of three (the moved children are non-increasing down the path, the chain towards the
// leaf): about a third fewer instructions per insert.  That holds whenever no two of the heap's elements and y share a key.
// TIES = true compares ranks without their tie field and selects.
//
// CHECK (plain form only): the round is computed in the plain form and committed only if that was exact.  Two ranks with one
// key are never both free of a tie field (it counts the equal keys before a candidate), so the plain round is exact unless
// one of the ranks it COMPARES has a non-zero tie field: the siblings along the pop's path, the ancestors of slot K, slots
// 1..7, the last element and y.  Their OR is at hand when the round's values are; `any(flag)` is the wave's OR over the
// inserting lanes (on the device a ballot, so every lane takes the same way).  If it says yes, nothing has been written
// -- every store and every update of r / last / q comes after it -- and the function returns false: the caller runs the round in
// the TIES form instead.  A heap that holds a group of equal keys meets one of its members in about one insert in ten.
struct NoAny {
    GD_RH_FN bool operator()(bool) const { return false; }
};
template <int K, bool TIES, bool CHECK = false, class Heap, class Any = NoAny>
GD_RH_FN bool insert(const Heap &H, unsigned int (&r)[8], unsigned int &last, unsigned int (&q)[4], const unsigned int y,
                     const unsigned int tm, const Any &any = Any()) {
    static_assert(K == 200, "ancestor chain of slot K");
    static_assert(!(TIES && CHECK), "the check belongs to the plain form");
    unsigned int seen = 0u;  // CHECK: OR of the pairs read along the path
    auto lt = [&](unsigned int a, unsigned int b) -> bool { return TIES ? key_lt(a, b, tm) : a < b; };
    auto larger = [&](unsigned int kl, unsigned int kr, bool &right) -> unsigned int {
        right = !lt(kr, kl);  // the right child unless it is smaller (src/binary_heap.hpp __adjust_heap)
        return TIES ? (right ? kr : kl) : umax(kl, kr);
    };
    int g[8];
    unsigned int ck[7];
    bool right0, right1;
    ck[0] = larger(r[2], r[3], right0);
    const unsigned int hl = right0 ? r[6] : r[4], hr = right0 ? r[7] : r[5];
    ck[1] = larger(hl, hr, right1);
    g[0] = 1;
    g[1] = 2 + (right0 ? 1 : 0);
    g[2] = 2 * g[1] + (right1 ? 1 : 0);
    const unsigned int q12 = q[0], q25 = q[1], q50 = q[2], q100 = q[3];
    // (two round trips: three levels below slot g[2] -- its children pair, both grandchildren pairs and all four
    // great-grandchildren pairs, seven dwords at constant offsets from one address -- then two levels below g[5].  Two, two and
    // one level were a round trip more per insert, and the inserts of the agent with the most candidates are the kernel's
    // duration: 452 -> 435 us)
    bool at12, at25, at50, at100;  // the pop's path goes through slot 12 / 25 / 50 / 100
    {
        const int g2 = g[2];
        const unsigned int pc = H.pair(g2), pl = H.pair(2 * g2), pr2 = H.pair(2 * g2 + 1);
        const unsigned int p0 = H.pair(4 * g2), p1 = H.pair(4 * g2 + 1), p2 = H.pair(4 * g2 + 2), p3 = H.pair(4 * g2 + 3);
        bool ra, rb, rc;
        ck[2] = larger(pc & 0xffffu, pc >> 16, ra);
        g[3] = 2 * g2 + (ra ? 1 : 0);
        const unsigned int pg = ra ? pr2 : pl;
        ck[3] = larger(pg & 0xffffu, pg >> 16, rb);
        g[4] = 2 * g[3] + (rb ? 1 : 0);
        const unsigned int pa = rb ? p1 : p0, pb = rb ? p3 : p2;
        const unsigned int pgg = ra ? pb : pa;
        ck[4] = larger(pgg & 0xffffu, pgg >> 16, rc);
        g[5] = 2 * g[4] + (rc ? 1 : 0);
        at12 = right0 && !right1 && !ra;
        at25 = at12 && rb;
        at50 = at25 && !rc;
        if (CHECK) seen |= pc | pg | pgg;
    }
    {
        const unsigned int pc = H.pair(g[5]), pl = H.pair(2 * g[5]), pr2 = H.pair(2 * g[5] + 1);
        bool ra, rb;
        ck[5] = larger(pc & 0xffffu, pc >> 16, ra);
        g[6] = 2 * g[5] + (ra ? 1 : 0);
        const unsigned int pg = ra ? pr2 : pl;
        ck[6] = larger(pg & 0xffffu, pg >> 16, rb);
        g[7] = 2 * g[6] + (rb ? 1 : 0);
        at100 = at50 && !ra;
        if (CHECK) seen |= pc | pg;
    }
    // the old last element climbs back from the leaf hole past every moved child that is smaller: like make_heap's sifts, the
    // value that ends up on level l is the median of (child moved from l - 1, child moved from l, last)
    unsigned int v[8];
    if (TIES) {
        bool c[7];
        GD_RH_UNROLL
        for (int l = 0; l < 7; l++) c[l] = lt(ck[l], last);
        GD_RH_UNROLL
        for (int l = 0; l < 8; l++) {
            if (l == 0) v[l] = c[0] ? last : ck[0];
            else if (l == 7) v[l] = c[6] ? ck[6] : last;
            else v[l] = c[l - 1] ? ck[l - 1] : (c[l] ? last : ck[l]);
        }
    } else {
        v[0] = umax(ck[0], last);
        GD_RH_UNROLL
        for (int l = 1; l < 7; l++) v[l] = med3(ck[l - 1], ck[l], last);
        v[7] = umin(ck[6], last);
    }
    if (CHECK) {
        seen |= r[1] | r[2] | r[3] | r[4] | r[5] | r[6] | r[7] | last | y | q12 | q25 | q50 | q100;
        if (any((seen & (tm * 0x10001u)) != 0u)) return false;
    }
    r[1] = v[0];
    r[2] = right0 ? r[2] : v[1];
    r[3] = right0 ? v[1] : r[3];
    {  // g[2] = 4 + 2 * right0 + right1: the pair (hl, hr) that level 1 chose from takes v[2] on the side of right1
        const unsigned int nl = right1 ? hl : v[2], nr = right1 ? v[2] : hr;
        r[4] = right0 ? r[4] : nl;
        r[5] = right0 ? r[5] : nr;
        r[6] = right0 ? nl : r[6];
        r[7] = right0 ? nr : r[7];
    }
    GD_RH_UNROLL
    for (int l = 3; l < 8; l++)
        if (l < 6 || g[l] < K) H.set(g[l], v[l]);  // levels 3..5 are always inside the heap
    // push_heap: the new element climbs from slot K along 100, 50, 25, 12, 6, 3, 1
    const unsigned int qv[7] = {r[1], r[3], r[6], at12 ? v[3] : q12, at25 ? v[4] : q25, at50 ? v[5] : q50, at100 ? v[6] : q100};
    constexpr int chain[7] = {1, 3, 6, 12, 25, 50, 100};
    if (TIES) {
        bool pp[7];
        GD_RH_UNROLL
        for (int u = 0; u < 7; u++) pp[u] = lt(qv[u], y);
        r[1] = pp[0] ? y : r[1];
        r[3] = pp[1] ? (pp[0] ? qv[0] : y) : r[3];
        r[6] = pp[2] ? (pp[1] ? qv[1] : y) : r[6];
        GD_RH_UNROLL
        for (int u = 3; u < 7; u++) {
            const unsigned int nv = pp[u - 1] ? qv[u - 1] : y;
            if (pp[u]) H.set(chain[u], nv);
            q[u - 3] = pp[u] ? nv : qv[u];  // (qv carries the pop's patch)
        }
        last = pp[6] ? qv[6] : y;
    } else {
        // chain position u receives its parent's value if that is below y, y if only its own is, and keeps its own
        // otherwise: the median of (parent, own, y), the chain being non-increasing towards the leaf
        r[1] = umax(qv[0], y);
        r[3] = med3(qv[0], qv[1], y);
        r[6] = med3(qv[1], qv[2], y);
        GD_RH_UNROLL
        for (int u = 3; u < 7; u++) {
            q[u - 3] = med3(qv[u - 1], qv[u], y);
            H.set(chain[u], q[u - 3]);
        }
        last = umin(qv[6], y);
    }
    return true;
}
// the mirrors of a column as it stands: for callers that do not keep them across rounds
template <class Heap>
GD_RH_FN void load_chain(const Heap &H, unsigned int (&q)[4]) {
    q[0] = H.get(12);
    q[1] = H.get(25);
    q[2] = H.get(50);
    q[3] = H.get(100);
}
template <int K, bool TIES, bool CHECK = false, class Heap, class Any = NoAny>
GD_RH_FN bool insert(const Heap &H, unsigned int (&r)[8], unsigned int &last, const unsigned int y, const unsigned int tm,
                     const Any &any = Any()) {
    unsigned int q[4];
    load_chain(H, q);
    return insert<K, TIES, CHECK>(H, r, last, q, y, tm, any);
}

// ---- where the equal-key form is needed ----
// A rank's tie field counts the equal keys EARLIER in road order and the candidates arrive in road order: the first member of
// a group of equal keys has field 0, every later one a non-zero field.  So while no element with a non-zero field is in the
// heap and the arriving candidate's field is 0, the heap and the candidate hold at most one member of every group, every
// comparison of the round is between different keys, and the plain round (TIES = false) is the key round bit for bit.  The
// TIES form is needed only from the arrival of a group's second member until the group has left the heap.
//
// TieTrack, per heap: `tg` -- the smallest of the ranks with a non-zero tie field that entered the heap since the track was
// last clear (NO_TIE: none); tl() -- such an element may be in the heap.  The root has the largest key, so once the root's key
// is below tg's, every element of the heap is below every tracked one: none of them is left, and the track clears.
constexpr unsigned int NO_TIE = 0xffffffffu;
struct TieTrack {
    unsigned int tg;
    GD_RH_FN bool tl() const { return tg != NO_TIE; }
};

// e if its tie field is non-zero, else NO_TIE: (e & tm) - 1 is all ones for a zero field and stays below the field otherwise
GD_RH_FN unsigned int tied_or_none(unsigned int e, unsigned int tm) { return e | ((e & tm) - 1u); }

// any rank with a non-zero tie field among `w`, ranks two per dword
template <int N>
GD_RH_FN bool any_tie(const unsigned int (&w)[N], const unsigned int tm) {
    unsigned int any = 0u;
    GD_RH_UNROLL
    for (int j = 0; j < N; j++) any |= w[j];
    return (any & (tm * 0x10001u)) != 0u;
}

// the track of a freshly filled heap (`w`: its K ranks, two per dword); make_heap only moves them
template <int N>
GD_RH_FN TieTrack track_of(const unsigned int (&w)[N], const unsigned int tm) {
    unsigned int lo = NO_TIE;
    GD_RH_UNROLL
    for (int j = 0; j < N; j++) lo = umin(lo, umin(tied_or_none(w[j] & 0xffffu, tm), tied_or_none(w[j] >> 16, tm)));
    return TieTrack{lo};
}

// any rank with a non-zero tie field among the first `left` of a block's eight candidates (`left` may be <= 0 or beyond 8)
GD_RH_FN bool block_has_tie(const unsigned int (&wd)[4], const int left, const unsigned int tm) {
    const unsigned int m = tm * 0x10001u;
    unsigned int any = 0u;
    GD_RH_UNROLL
    for (int j = 0; j < 4; j++) any |= left > 2 * j + 1 ? wd[j] & m : (left == 2 * j + 1 ? wd[j] & tm : 0u);
    return any != 0u;
}

// The rounds of one block: candidates wd (eight ranks, the first `left` of them this heap's) through the entry test and the
// insert, in one of three forms that the wave chooses per block:
//   PLAIN    no heap of the wave has a track and no candidate of the block a non-zero tie field: nothing to maintain;
//   TIES     some candidate of the block has a non-zero tie field: the equal-key form throughout, which maintains the track;
//   CHECKED  some heap has a track, the candidates are free: every round in the plain form unless it meets a tied rank
//            (insert's CHECK).  The entry test is exact in the plain form: y's tie field is 0, so y is the first of its group
//            in road order and no member of it has come yet.
// `round` is one of the eight; both return the number of inserts.
enum Form { PLAIN, TIES, CHECKED };
template <int K, Form F, class Heap, class Any = NoAny>
GD_RH_FN int round(const Heap &H, unsigned int (&r)[8], unsigned int &last, unsigned int (&q)[4], const unsigned int y,
                   const bool mine, const unsigned int tm, TieTrack &t, const Any &any = Any()) {
    if (!(mine && (F == TIES ? key_lt(y, r[1], tm) : y < r[1]))) return 0;
    if (F == TIES) {
        insert<K, true>(H, r, last, q, y, tm);
        t.tg = umin(t.tg, tied_or_none(y, tm));
    } else if (F == CHECKED) {
        if (!insert<K, false, true>(H, r, last, q, y, tm, any)) insert<K, true>(H, r, last, q, y, tm);
    } else {
        insert<K, false>(H, r, last, q, y, tm);
    }
    return 1;
}
template <int K, Form F, class Heap, class Any = NoAny>
GD_RH_FN int round(const Heap &H, unsigned int (&r)[8], unsigned int &last, const unsigned int y, const bool mine,
                   const unsigned int tm, TieTrack &t, const Any &any = Any()) {
    unsigned int q[4];
    load_chain(H, q);
    return round<K, F>(H, r, last, q, y, mine, tm, t, any);
}
// the end of a block that ran with a track: the root below every tracked rank means none of them is left
GD_RH_FN void block_end(const unsigned int root, const unsigned int tm, TieTrack &t) {
    if (key_lt(root, t.tg, tm)) t.tg = NO_TIE;
}
GD_RH_FN unsigned int block_rank(const unsigned int (&wd)[4], const int k) { return (k & 1) ? wd[k >> 1] >> 16 : wd[k >> 1] & 0xffffu; }
template <int K, Form F, class Heap, class Any = NoAny>
GD_RH_FN int block_rounds(const Heap &H, unsigned int (&r)[8], unsigned int &last, unsigned int (&q)[4],
                          const unsigned int (&wd)[4], const int left, const unsigned int tm, TieTrack &t, const Any &any = Any()) {
    int ins = 0;
    GD_RH_UNROLL
    for (int k = 0; k < 8; k++) ins += round<K, F>(H, r, last, q, block_rank(wd, k), k < left, tm, t, any);
    if (F != PLAIN) block_end(r[1], tm, t);
    return ins;
}
template <int K, Form F, class Heap, class Any = NoAny>
GD_RH_FN int block_rounds(const Heap &H, unsigned int (&r)[8], unsigned int &last, const unsigned int (&wd)[4], const int left,
                          const unsigned int tm, TieTrack &t, const Any &any = Any()) {
    unsigned int q[4];
    load_chain(H, q);
    return block_rounds<K, F>(H, r, last, q, wd, left, tm, t, any);
}

}  // namespace rank_heap
}  // namespace gd
