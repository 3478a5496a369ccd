// Host model of k_knn_replay's rounds: runs csrc/rank_heap.hpp (the very code the kernel runs: fill, make_heap, the insert in
// its plain, its checked and its equal-key form, the tie track and the per-block test) for a model "wave" of several lanes with
// the OR-ed choice of the form per block of eight candidates (and per round in the checked form), the way the kernel's loop
// makes it, against the reference algorithm on
// KEYS: std::make_heap over the first K candidates, then per candidate `key < heap[0]`, std::pop_heap, replace last,
// std::push_heap, all with the strict key comparator.  The whole heap array and the root are compared after every tile of 32
// candidates and at the end.  In every block that runs in the plain form the model also asserts what makes that form exact:
// no two elements of heap + the block's candidates share a key; in the checked form, that a round told to step back has
// changed nothing and that a round committed in the plain form equals the equal-key form's.
// Prints one line per kind of input: "<name> waves <n> bad <m> inv_bad <i> ties_blocks <t> checked_blocks <c> blocks <b>
// checked_inserts <n> redone <n>".
// Usage: replay_rounds_model <waves per kind>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../gpudrive_lab_amd/csrc/rank_heap.hpp"

namespace {

namespace rh = gd::rank_heap;
constexpr int K = 200;
constexpr int NPAIR = rh::NPAIR;
constexpr int TILE = 32;
constexpr int LANES = 4;

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
int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }  // inclusive

// the two rank formats (map_obs_rank.hip RankGeo): tie field of 5 bits and up to 1272 candidates, 4 bits and up to 2552
struct Format { int rsh, nmax; };
constexpr Format STANDARD{5, 1272}, LONG{4, 2552};

// ranks the way k_knn_rank forms them: (keys below + 1) << rsh | equal keys earlier in road order
std::vector<uint16_t> ranks_of(const std::vector<long> &keys, int rsh) {
    const int n = (int)keys.size();
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a < b; });
    std::vector<uint16_t> e(n);
    for (int s = 0; s < n;) {
        int t = s;
        while (t < n && keys[idx[t]] == keys[idx[s]]) t++;
        for (int m = s; m < t; m++) {
            if (m - s >= (1 << rsh) || s + 1 >= (1 << (16 - rsh))) { std::fprintf(stderr, "generator: a rank does not fit\n"); std::abort(); }
            e[idx[m]] = (uint16_t)(((s + 1) << rsh) | (m - s));
        }
        s = t;
    }
    return e;
}

// ---- inputs ----
enum Kind { FREE, GROUPS, ROOT, STAY, LATE, FAIL, FIRSTK, ALLEQ, IDLE, NKINDS };
const char *const NAMES[NKINDS] = {"tie_free", "random_groups", "meet_at_root", "stay_to_end", "after_eviction", "fails_entry",
                                   "inside_first_k", "all_equal", "idle"};

// distinct keys, all multiples of 4 (a group takes the key of one of its members + 1: distinct from every other key)
// trend 0: random order; 1: strictly descending with noise (every candidate is an insert and climbs to the root within about
// K inserts); 2: descending with noise over some 300 positions (most candidates are inserts)
std::vector<long> base_keys(int n, int trend) {
    std::vector<long> k(n);
    for (int a = 0; a < n; a++) {
        const long v = trend == 0 ? (long)(rnd() % 1000000u) : trend == 1 ? (long)(n - a) * 16 + rnd() % 16 : (long)(n - a) * 16 + rnd() % 4800;
        k[a] = (v * 4096 + a) * 4;
    }
    return k;
}

void make_group(std::vector<long> &k, const std::vector<int> &pos) {
    if (pos.size() < 2) return;  // (no room left around the place drawn)
    const long key = k[pos[0]] + 1;
    for (int p : pos) k[p] = key;
}

std::vector<int> distinct_positions(int members, int lo, int hi, std::vector<char> &used) {  // in [lo, hi], not used before
    std::vector<int> pos;
    for (int tries = 0; (int)pos.size() < members && tries < 1000; tries++) {
        const int p = rnd_in(lo, hi);
        if (!used[p]) { used[p] = 1; pos.push_back(p); }
    }
    std::sort(pos.begin(), pos.end());
    return pos;
}

std::vector<long> keys_of(Kind kind, const Format f, int &n) {
    const int most = (1 << f.rsh);  // members a rank can count
    n = rnd() % 4 == 0 ? f.nmax - (int)(rnd() % 40) : rnd_in(K, f.nmax);
    if (kind == LATE) n = std::max(n, K + 700);
    if (kind == IDLE) { n = rnd_in(0, K - 1); return base_keys(n, 0); }
    std::vector<char> used(n, 0);
    std::vector<long> k;
    switch (kind) {
    case FREE: k = base_keys(n, rnd() % 3); break;
    case GROUPS: {
        k = base_keys(n, rnd() % 3);
        for (int q = 1 + rnd() % 8; q > 0; q--) make_group(k, distinct_positions(rnd_in(2, std::min(12, most)), 0, n - 1, used));
        break;
    }
    case ROOT: {  // members close together on a descending trend: they reach the root together and leave in consecutive pops
        k = base_keys(n, 1 + rnd() % 2);
        for (int q = 1 + rnd() % 6; q > 0; q--) {
            const int p = rnd_in(0, n - 1);
            make_group(k, distinct_positions(rnd_in(2, 6), p, std::min(n - 1, p + 40), used));
        }
        break;
    }
    case STAY: {  // below every other key: once in, a member stays to the end
        k = base_keys(n, rnd() % 3);
        for (int q = 1 + rnd() % 3; q > 0; q--) {
            const std::vector<int> pos = distinct_positions(rnd_in(2, std::min(12, most)), 0, n - 1, used);
            for (int p : pos) k[p] = -4l * q + 1;
        }
        break;
    }
    case LATE: {  // strictly descending: a member is evicted about K inserts after it came; one more member comes long after
        k = base_keys(n, 1);
        for (int q = 1 + rnd() % 3; q > 0; q--) {
            const int p = rnd_in(0, n - 650);
            std::vector<int> pos = distinct_positions(rnd_in(2, 5), p, p + 30, used);
            const std::vector<int> late = distinct_positions(rnd_in(1, 2), p + 400, n - 1, used);
            pos.insert(pos.end(), late.begin(), late.end());
            make_group(k, pos);
        }
        break;
    }
    case FAIL: {  // a key above (nearly) every other: the first member is among the first K or evicted soon, the later ones fail the entry test
        k = base_keys(n, 0);
        for (int q = 1 + rnd() % 4; q > 0; q--) {
            std::vector<int> pos = distinct_positions(1, 0, std::min(n - 1, K + 50), used);
            const std::vector<int> later = distinct_positions(rnd_in(1, 6), pos.empty() ? 0 : pos[0], n - 1, used);
            pos.insert(pos.end(), later.begin(), later.end());
            const long key = (1000000l * 4096 + 5000 * (long)rnd_in(-3, 1)) * 4 + 4 * q + 1;
            for (int p : pos) k[p] = key;
        }
        break;
    }
    case FIRSTK: {
        k = base_keys(n, rnd() % 3);
        for (int q = 1 + rnd() % 6; q > 0; q--) make_group(k, distinct_positions(rnd_in(2, std::min(12, most)), 0, K - 1, used));
        break;
    }
    case ALLEQ: {  // every key shared by as many candidates as a rank can count (one more sends the agent to the fallback path
                   // before the replay), the members anywhere
        k.resize(n);
        for (int a = 0; a < n; a++) k[a] = a / most;
        for (int a = n - 1; a > 0; a--) std::swap(k[a], k[rnd() % (a + 1)]);
        break;
    }
    default: std::abort();
    }
    return k;
}

// ---- the model wave ----
struct Lane {
    Format f{};
    int n = 0;
    bool on = false, has_tie = false;
    unsigned tm = 0;
    std::vector<long> keys;
    std::vector<uint16_t> E;  // the ranks, then slack (whatever is there)
    uint32_t col[NPAIR];
    unsigned int r[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
    rh::TieTrack tt{rh::NO_TIE};
    std::vector<int> ref;  // the reference's heap: candidate indices
    int ref_done = 0;      // candidates the reference has seen
};

void reference_advance(Lane &L, int upto) {
    auto cmp = [&](int a, int b) { return L.keys[a] < L.keys[b]; };
    if (L.ref_done == 0) {
        L.ref.resize(K);
        std::iota(L.ref.begin(), L.ref.end(), 0);
        std::make_heap(L.ref.begin(), L.ref.end(), cmp);
        L.ref_done = K;
    }
    for (; L.ref_done < upto; L.ref_done++) {
        const int c = L.ref_done;
        if (L.keys[c] < L.keys[L.ref[0]]) {
            std::pop_heap(L.ref.begin(), L.ref.end(), cmp);
            L.ref.back() = c;
            std::push_heap(L.ref.begin(), L.ref.end(), cmp);
        }
    }
}

unsigned int model_slot(const Lane &L, int s) {  // the heap array as the kernel writes it out
    return s < 8 ? L.r[s] : s == K ? L.last : HostHeap{const_cast<uint32_t *>(L.col)}.get(s);
}

int compare(Lane &L, int upto) {
    reference_advance(L, upto);
    int bad = 0;
    for (int s = 1; s <= K; s++) bad += model_slot(L, s) != L.E[L.ref[s - 1]];
    bad += L.r[1] != L.E[L.ref[0]];  // the root (the checkpoint the kernel records)
    const HostHeap H{L.col};
    bad += H.get(0) != 0 || H.get(K) != 0 || H.get(K + 1) != 0;  // slot K lives in `last` during the rounds
    for (int j = K / 2 + 1; j < NPAIR; j++) bad += L.col[j] != 0;
    return bad;
}

// what makes the plain form exact: heap + the block's candidates hold no two ranks with the same high part
bool distinct_keys(const Lane &L, const unsigned int (&wd)[4], int left) {
    std::vector<unsigned> hi;
    for (int s = 1; s <= K; s++) hi.push_back(model_slot(L, s) >> L.f.rsh);
    for (int k = 0; k < 8 && k < left; k++) hi.push_back(((k & 1) ? wd[k >> 1] >> 16 : wd[k >> 1] & 0xffffu) >> L.f.rsh);
    std::sort(hi.begin(), hi.end());
    return std::adjacent_find(hi.begin(), hi.end()) == hi.end();
}

struct Tally { long waves = 0, bad = 0, inv_bad = 0, ties_blocks = 0, checked_blocks = 0, blocks = 0, checked_inserts = 0, redone = 0; };

void run_wave(Lane (&W)[LANES], Tally &t) {
    int nmax = 0;
    bool wave_ties = false;
    for (Lane &L : W) {
        nmax = std::max(nmax, L.n);
        wave_ties |= L.on && L.has_tie;
    }
    long bad = 0, inv_bad = 0;
    // the fill, the track of the first K, make_heap in the form the wave takes
    unsigned int w[LANES][K / 2];
    bool any_first = false;
    for (int l = 0; l < LANES; l++) {
        Lane &L = W[l];
        for (int k = 0; k < K / 2; k++) w[l][k] = (uint32_t)L.E[2 * k] | ((uint32_t)L.E[2 * k + 1] << 16);
        std::memset(L.col, 0xff, sizeof(L.col));
        rh::fill_pairs<K>(HostHeap{L.col}, w[l]);
        any_first |= L.on && rh::any_tie(w[l], L.tm);
    }
    if (wave_ties && any_first)
        for (int l = 0; l < LANES; l++) {
            W[l].tt = rh::track_of(w[l], W[l].tm);
            if (!W[l].on) W[l].tt.tg = rh::NO_TIE;
        }
    bool heap_ties = false;
    for (Lane &L : W) heap_ties |= L.tt.tl();
    for (Lane &L : W) {
        const HostHeap H{L.col};
        if (L.on) {
            if (heap_ties) rh::make_heap<K, true>(H, L.tm);
            else rh::make_heap<K, false>(H, L.tm);
        }
        for (int j = 1; j < 8; j++) L.r[j] = H.get(j);
        L.last = H.get(K);
        H.set(K, 0u);
        if (L.on) bad += compare(L, K) != 0;
    }
    // the rounds: per block of eight candidates one form for the whole wave
    for (int p0 = K; p0 < nmax; p0 += TILE) {
        for (int pb = p0; pb < std::min(p0 + TILE, nmax); pb += 8) {
            unsigned int wd[LANES][4];
            bool full = false, tracked = false;
            for (int l = 0; l < LANES; l++) {
                Lane &L = W[l];
                for (int j = 0; j < 4; j++) wd[l][j] = (uint32_t)L.E[pb + 2 * j] | ((uint32_t)L.E[pb + 2 * j + 1] << 16);
                full |= wave_ties && L.on && rh::block_has_tie(wd[l], L.n - pb, L.tm);
                tracked |= wave_ties && L.tt.tl();
            }
            if (full) {
                for (int l = 0; l < LANES; l++)
                    rh::block_rounds<K, rh::TIES>(HostHeap{W[l].col}, W[l].r, W[l].last, wd[l], W[l].n - pb, W[l].tm, W[l].tt);
            } else if (tracked) {
                // the checked form, round by round: the wave's OR over the inserting lanes first (a call that is told "yes" must
                // leave the lane as it was), then the round itself; a round that was committed in the plain form must equal
                // the equal-key form's
                for (int k = 0; k < 8; k++) {
                    bool any = false;
                    for (int l = 0; l < LANES; l++) {
                        Lane &L = W[l];
                        const unsigned int y = rh::block_rank(wd[l], k);
                        if (!(k < L.n - pb && y < L.r[1])) continue;
                        const Lane before = L;
                        bool flag = false;
                        const bool done = rh::insert<K, false, true>(HostHeap{L.col}, L.r, L.last, y, L.tm, [&](bool f) { flag = f; return true; });
                        inv_bad += done || std::memcmp(before.col, L.col, sizeof(L.col)) != 0 || std::memcmp(before.r, L.r, sizeof(L.r)) != 0 || before.last != L.last;
                        any |= flag;
                    }
                    for (int l = 0; l < LANES; l++) {
                        Lane &L = W[l];
                        const unsigned int y = rh::block_rank(wd[l], k);
                        uint32_t col2[NPAIR];
                        unsigned int r2[8], last2 = L.last;
                        std::memcpy(col2, L.col, sizeof(col2));
                        std::memcpy(r2, L.r, sizeof(r2));
                        const int ins = rh::round<K, rh::CHECKED>(HostHeap{L.col}, L.r, L.last, y, k < L.n - pb, L.tm, L.tt, [&](bool) { return any; });
                        if (ins) {
                            rh::insert<K, true>(HostHeap{col2}, r2, last2, y, L.tm);
                            inv_bad += std::memcmp(col2, L.col, sizeof(col2)) != 0 || std::memcmp(r2, L.r, sizeof(r2)) != 0 || last2 != L.last;
                            t.checked_inserts++;
                            t.redone += any;
                        }
                    }
                }
                for (Lane &L : W) rh::block_end(L.r[1], L.tm, L.tt);
            } else {
                for (int l = 0; l < LANES; l++) {
                    Lane &L = W[l];
                    if (L.on) inv_bad += !distinct_keys(L, wd[l], L.n - pb);
                    rh::block_rounds<K, rh::PLAIN>(HostHeap{L.col}, L.r, L.last, wd[l], L.n - pb, L.tm, L.tt);
                }
            }
            t.blocks += wave_ties;
            t.ties_blocks += full;
            t.checked_blocks += !full && tracked;
        }
        for (Lane &L : W)
            if (L.on && p0 < L.n) bad += compare(L, std::min(L.n, p0 + TILE)) != 0;
    }
    for (Lane &L : W)
        if (L.on) bad += compare(L, L.n) != 0;
    t.waves++;
    t.bad += bad != 0;
    t.inv_bad += inv_bad != 0;
}

void make_lane(Lane &L, Kind kind, const Format f) {
    L = Lane{};
    L.f = f;
    L.tm = (1u << f.rsh) - 1u;
    L.keys = keys_of(kind, f, L.n);
    L.on = L.n >= K;
    L.E = ranks_of(L.keys, f.rsh);
    for (uint16_t e : L.E) L.has_tie |= (e & L.tm) != 0;
    // slack: the kernel reads whole blocks up to its wave's longest agent and two blocks ahead; what is there must not matter
    const int slack_kind = rnd() % 3;
    while ((int)L.E.size() < LONG.nmax + 24) L.E.push_back(slack_kind == 0 ? 0 : slack_kind == 1 ? 0xffff : (uint16_t)rnd());
}

}  // namespace

int main(int argc, char **argv) {
    const int nw = argc > 1 ? std::atoi(argv[1]) : 300;
    long bad = 0;
    for (int kind = FREE; kind < IDLE; kind++) {
        Tally t;
        for (int c = 0; c < nw; c++) {
            Lane W[LANES];
            const Format f = c % 2 ? LONG : STANDARD;  // lane 0 takes both formats in turn
            make_lane(W[0], (Kind)kind, f);
            if (kind == FREE) {  // a wave without equal keys, beside idle lanes and slack of any content: never the equal-key form
                make_lane(W[1], FREE, rnd() % 2 ? LONG : STANDARD);
                make_lane(W[2], rnd() % 2 ? FREE : IDLE, f);
                make_lane(W[3], IDLE, STANDARD);
            } else {  // a lane without ties beside the tied one, a lane of any kind (either format), an idle or a short one
                make_lane(W[1], FREE, f);
                make_lane(W[2], (Kind)(rnd() % IDLE), rnd() % 2 ? LONG : STANDARD);
                make_lane(W[3], rnd() % 2 ? IDLE : FREE, STANDARD);
                if (W[3].on) { W[3].n = std::min(W[3].n, K + (int)(rnd() % 64)); W[3].keys.resize(W[3].n); W[3].E = ranks_of(W[3].keys, W[3].f.rsh); W[3].E.resize(LONG.nmax + 24, 0xffff); }
            }
            std::swap(W[0], W[rnd() % LANES]);  // the lane under test anywhere in the wave
            run_wave(W, t);
        }
        std::printf("%s waves %ld bad %ld inv_bad %ld ties_blocks %ld checked_blocks %ld blocks %ld checked_inserts %ld redone %ld\n", NAMES[kind],
                    t.waves, t.bad, t.inv_bad, t.ties_blocks, t.checked_blocks, t.blocks, t.checked_inserts, t.redone);
        bad += t.bad + t.inv_bad;
        if (kind == FREE) bad += t.ties_blocks + t.checked_blocks;
    }
    std::printf("bad_access %ld\n", HostHeap::bad_access);
    return bad + HostHeap::bad_access != 0;
}
