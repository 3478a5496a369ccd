// Host model of k_knn_replay's prologue: runs csrc/rank_heap.hpp (the very code the kernel runs) against std::make_heap with
// the rank comparator and against the plain slot-by-slot fill.  Prints one line per check: "<name> cases <n> bad <m>".
// Usage: replay_heap_model <random cases per kind>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/rank_heap.hpp"

namespace {

constexpr int K = 200;
constexpr int NPAIR = gd::rank_heap::NPAIR;

struct HostHeap {  // one column, stride 1
    uint32_t *p;
    uint32_t pair(int j) const { check(j); return p[j]; }
    uint32_t get(int g) const { check(g >> 1); return (p[g >> 1] >> ((g & 1) * 16)) & 0xffffu; }
    void set(int g, uint32_t v) const {
        check(g >> 1);
        if (g < 1 || g > K || v > 0xffffu) bad_access++;
        const int sh = (g & 1) * 16;
        p[g >> 1] = (p[g >> 1] & ~(0xffffu << sh)) | (v << sh);
    }
    void set_pair(int j, uint32_t v) const { check(j); p[j] = v; }
    static void check(int j) { if (j < 0 || j >= NPAIR) { bad_access++; std::abort(); } }
    static long bad_access;
};
long HostHeap::bad_access = 0;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

// ranks of K keys the way k_knn_rank forms them: (keys below + 1) << rsh | equal keys before.  A key with more equal ones
// before it than the field counts never reaches the replay (the agent falls back); `wrap` folds the count so that arrays with
// more equal keys than that -- up to all K equal -- still exercise the comparator (several slots then hold one value).
std::vector<uint16_t> ranks_of(const std::vector<int> &keys, int rsh) {
    std::vector<uint16_t> e(K);
    for (int a = 0; a < K; a++) {
        int less = 0, eq = 0;
        for (int b = 0; b < K; b++) {
            less += keys[b] < keys[a];
            eq += b < a && keys[b] == keys[a];
        }
        e[a] = (uint16_t)(((less + 1) << rsh) | (eq & ((1 << rsh) - 1)));
    }
    return e;
}

void reference_fill(const std::vector<uint16_t> &e, uint32_t *col) {
    std::memset(col, 0, sizeof(uint32_t) * NPAIR);
    HostHeap H{col};
    for (int s = 1; s <= K; s++) H.set(s, e[s - 1]);
}

// fill + make_heap through rank_heap.hpp; returns the number of differences to std::make_heap / the plain fill
template <bool TIES>
int run_case(const std::vector<uint16_t> &e, unsigned tm, int &fill_bad) {
    uint32_t col[NPAIR], ref[NPAIR];
    std::memset(col, 0xff, sizeof(col));  // the fill must write every dword
    unsigned int w[K / 2];
    for (int k = 0; k < K / 2; k++) w[k] = (uint32_t)e[2 * k] | ((uint32_t)e[2 * k + 1] << 16);
    HostHeap H{col};
    gd::rank_heap::fill_pairs<K>(H, w);
    reference_fill(e, ref);
    fill_bad += std::memcmp(col, ref, sizeof(col)) != 0;
    gd::rank_heap::make_heap<K, TIES>(H, tm);
    std::vector<uint16_t> want(e);
    std::make_heap(want.begin(), want.end(), [tm](uint16_t a, uint16_t b) { return ((unsigned)a | tm) < (unsigned)b; });
    int bad = 0;
    for (int s = 1; s <= K; s++) bad += H.get(s) != want[s - 1];
    bad += H.get(0) != 0 || H.get(K + 1) != 0;
    for (int j = K / 2 + 1; j < NPAIR; j++) bad += col[j] != 0;  // the pairs beyond the heap
    return bad;
}

struct Tally { const char *name; long cases = 0, bad = 0, fill_bad = 0; };

void run(Tally &t, const std::vector<int> &keys, bool tie_free) {
    for (int rsh : {5, 4}) {
        const unsigned tm = (1u << rsh) - 1u;
        const std::vector<uint16_t> e = ranks_of(keys, rsh);
        int fb = 0;
        t.bad += run_case<true>(e, tm, fb) != 0;
        if (tie_free) t.bad += run_case<false>(e, tm, fb) != 0;  // the tie-free form is taken only by waves without equal keys
        t.fill_bad += fb != 0;
        t.cases++;
    }
}

}  // namespace

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 10000;
    std::vector<int> keys(K);
    Tally distinct{"distinct"}, groups{"equal_groups"}, equal{"all_equal"}, sorted{"sorted"}, reversed{"reverse_sorted"}, few{"few_keys"};
    for (int c = 0; c < n; c++) {  // a random permutation: no equal keys
        for (int a = 0; a < K; a++) keys[a] = a;
        for (int a = K - 1; a > 0; a--) std::swap(keys[a], keys[rnd() % (a + 1)]);
        run(distinct, keys, true);
    }
    for (int c = 0; c < n; c++) {  // several groups of equal keys (2..12 members each) among distinct ones
        for (int a = 0; a < K; a++) keys[a] = 1000 + a;
        const int ngroups = 1 + rnd() % 8;
        for (int q = 0; q < ngroups; q++) {
            const int members = 2 + rnd() % 11, key = 1000 + rnd() % K;
            for (int m = 0; m < members; m++) keys[rnd() % K] = key;
        }
        for (int a = K - 1; a > 0; a--) std::swap(keys[a], keys[rnd() % (a + 1)]);
        run(groups, keys, false);
    }
    for (int c = 0; c < n / 10 + 1; c++) {  // a handful of keys: long runs of equal ones
        const int nk = 1 + rnd() % 6;
        for (int a = 0; a < K; a++) keys[a] = rnd() % nk;
        run(few, keys, false);
    }
    for (int a = 0; a < K; a++) keys[a] = 7;
    run(equal, keys, false);
    for (int a = 0; a < K; a++) keys[a] = a;
    run(sorted, keys, true);
    for (int a = 0; a < K; a++) keys[a] = a / 3;  // sorted with equal neighbours
    run(sorted, keys, false);
    for (int a = 0; a < K; a++) keys[a] = K - a;
    run(reversed, keys, true);
    for (int a = 0; a < K; a++) keys[a] = (K - a) / 3;
    run(reversed, keys, false);
    long bad = HostHeap::bad_access;
    for (const Tally *t : {&distinct, &groups, &few, &equal, &sorted, &reversed}) {
        std::printf("%s cases %ld bad %ld fill_bad %ld\n", t->name, t->cases, t->bad, t->fill_bad);
        bad += t->bad + t->fill_bad;
    }
    std::printf("bad_access %ld\n", HostHeap::bad_access);
    return bad != 0;
}
