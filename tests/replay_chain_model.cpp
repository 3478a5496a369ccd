// Host model of the registers k_knn_replay keeps across its rounds: csrc/rank_heap.hpp's rounds with the chain mirrors `q`
// (slots 12, 25, 50, 100: with 1, 3, 6 the ancestors of slot K that every push climbs), held across every round, every block
// and every change of form, the way the kernel holds them, for model "waves" of four lanes that choose the form per block of
// eight candidates exactly as the kernel's loop does.  (Generators and the reference on keys as in replay_rounds_model.cpp,
// which checks the forms themselves per tile; this one checks after EVERY round.)
//
// After every round, for every lane:
//   - q[u] equals the column's slot 12 / 25 / 50 / 100: the column stays authoritative, the mirrors only follow;
//   - the whole heap array and the root equal the reference's -- std::make_heap over the first K candidates, then per candidate
//     `key < heap[0]`, std::pop_heap, replace last, std::push_heap with the strict key comparator -- and a round inserts exactly
//     when the reference does;
//   - the slots that must hold 0 do: 0, K (its element lives in `last`), K + 1 and the pairs K/2 + 1 .. 127.
// A round of the checked form that is told to step back must leave r, last, q and the column untouched (inv_bad).
// After every block, three copies of each lane must agree in column, r, last and tie track (wrap_bad): the one run round by
// round through round(.., q, ..), one run through block_rounds(.., q, ..) and one through the signatures without `q`, which load
// the mirrors from the column for every call.
// The pop's path is followed independently on the reference's heap (keys only) and counted where it passes through slot 12,
// 25, 50, 100: those are the rounds in which a mirror is patched by the pop.  A kind of input whose path never passes through
// one of them fails.
// Prints one line per kind of input:
//   "<name> waves <n> bad <b> inv_bad <i> mirror_bad <m> wrap_bad <w> rounds <r> inserts <n> via12 <n> via25 <n> via50 <n>
//    via100 <n> ties_blocks <t> checked_blocks <c> stepped_back <s>"
// Usage: replay_chain_model <waves per kind>
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
constexpr int CHAIN[4] = {12, 25, 50, 100};

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

uint64_t rng_state = 0x2545f4914f6cdd1dull;
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

// ---- inputs (the kinds of replay_rounds_model.cpp; IDLE here is a kind of wave: one agent beside three idle lanes) ----
enum Kind { FREE, GROUPS, ROOT, STAY, LATE, FAIL, FIRSTK, ALLEQ, IDLE, NKINDS };
const char *const NAMES[NKINDS] = {"tie_free", "random_groups", "meet_at_root", "stay_to_end", "after_eviction", "fails_entry",
                                   "inside_first_k", "all_equal", "idle_lanes"};

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
    case ALLEQ: {  // every key shared by as many candidates as a rank can count, the members anywhere
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
struct State {  // what a lane of the kernel holds during the rounds
    uint32_t col[NPAIR];
    unsigned int r[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0, q[4] = {0, 0, 0, 0};
    rh::TieTrack tt{rh::NO_TIE};
};
bool same(const State &a, const State &b, bool with_q) {
    return std::memcmp(a.col, b.col, sizeof(a.col)) == 0 && std::memcmp(a.r + 1, b.r + 1, 7 * sizeof(unsigned int)) == 0 && a.last == b.last &&
           a.tt.tg == b.tt.tg && (!with_q || std::memcmp(a.q, b.q, sizeof(a.q)) == 0);
}

struct Lane {
    Format f{};
    int n = 0;
    bool on = false, has_tie = false;
    unsigned tm = 0;
    std::vector<long> keys;
    std::vector<uint16_t> E;  // the ranks, then slack (whatever is there)
    State s;                  // round by round, mirrors held
    State sb;                 // block by block, mirrors held
    State sw;                 // block by block through the signatures without mirrors
    std::vector<int> ref;     // the reference's heap: candidate indices
    std::vector<char> told;   // the checked form: what the wave's OR told this lane in each of its inserting rounds of the block
};

struct Tally {
    long waves = 0, bad = 0, inv_bad = 0, mirror_bad = 0, wrap_bad = 0, rounds = 0, inserts = 0, via[4] = {0, 0, 0, 0}, ties_blocks = 0,
         checked_blocks = 0, stepped_back = 0;
};

// the reference's round for candidate c; the pop's path (the hole's way down over the K - 1 elements that stay,
// __adjust_heap: the right child unless it is smaller) is followed on keys before the pop
bool reference_round(Lane &L, int c, Tally &t) {
    auto cmp = [&](int a, int b) { return L.keys[a] < L.keys[b]; };
    if (!(L.keys[c] < L.keys[L.ref[0]])) return false;
    const int len = K - 1;  // slots 1..K-1
    for (int g = 1;;) {
        int child;
        if (2 * g + 1 <= len) child = cmp(L.ref[2 * g], L.ref[2 * g - 1]) ? 2 * g : 2 * g + 1;  // slot s is ref[s - 1]
        else if (2 * g == len) child = 2 * g;
        else break;
        g = child;
        for (int u = 0; u < 4; u++) t.via[u] += g == CHAIN[u];
    }
    std::pop_heap(L.ref.begin(), L.ref.end(), cmp);
    L.ref.back() = c;
    std::push_heap(L.ref.begin(), L.ref.end(), cmp);
    return true;
}

unsigned int model_slot(const State &S, int s) {  // the heap array as the kernel writes it out
    return s < 8 ? S.r[s] : s == K ? S.last : HostHeap{const_cast<uint32_t *>(S.col)}.get(s);
}

int mirrors_off(const State &S) {
    const HostHeap H{const_cast<uint32_t *>(S.col)};
    int bad = 0;
    for (int u = 0; u < 4; u++) bad += S.q[u] != H.get(CHAIN[u]);
    return bad;
}

int heap_off(const Lane &L) {
    const State &S = L.s;
    int bad = 0;
    for (int s = 1; s <= K; s++) bad += model_slot(S, s) != L.E[L.ref[s - 1]];
    bad += S.r[1] != L.E[L.ref[0]];  // the root (the checkpoint the kernel records)
    const HostHeap H{const_cast<uint32_t *>(S.col)};
    bad += H.get(0) != 0 || H.get(K) != 0 || H.get(K + 1) != 0;  // slot K lives in `last` during the rounds
    for (int j = K / 2 + 1; j < NPAIR; j++) bad += S.col[j] != 0;
    return bad;
}

struct Told {  // the checked form's `any` for a copy that runs a whole block: the answers the round-by-round copy got, in order
    const std::vector<char> *v;
    mutable size_t at;
    bool operator()(bool) const {
        if (at >= v->size()) { overrun++; return false; }  // the copy inserts where the round-by-round one did not: counted as wrap_bad
        return (*v)[at++] != 0;
    }
    static long overrun;
};
long Told::overrun = 0;

template <rh::Form F>
void run_block(Lane (&W)[LANES], const unsigned int (&wd)[LANES][4], int pb, Tally &t, long &bad, long &inv_bad, long &mirror_bad, long &wrap_bad) {
    for (Lane &L : W) L.told.clear();
    for (int k = 0; k < 8; k++) {
        bool any = false;
        if (F == rh::CHECKED) {  // the wave's OR over the inserting lanes: a call that is told "yes" must leave the lane as it was
            for (int l = 0; l < LANES; l++) {
                Lane &L = W[l];
                const unsigned int y = rh::block_rank(wd[l], k);
                if (!(k < L.n - pb && y < L.s.r[1])) continue;
                const State before = L.s;
                bool flag = false;
                const bool done = rh::insert<K, false, true>(HostHeap{L.s.col}, L.s.r, L.s.last, L.s.q, y, L.tm, [&](bool f) { flag = f; return true; });
                inv_bad += done || !same(before, L.s, true);
                any |= flag;
            }
        }
        for (int l = 0; l < LANES; l++) {
            Lane &L = W[l];
            const unsigned int y = rh::block_rank(wd[l], k);
            const int ins = rh::round<K, F>(HostHeap{L.s.col}, L.s.r, L.s.last, L.s.q, y, k < L.n - pb, L.tm, L.s.tt, [&](bool) { return any; });
            if (F == rh::CHECKED && ins) {
                L.told.push_back(any);
                t.stepped_back += any;
            }
            mirror_bad += mirrors_off(L.s) != 0;
            if (L.on && pb + k < L.n) {
                const bool ref_ins = reference_round(L, pb + k, t);
                bad += (ins != 0) != ref_ins || heap_off(L) != 0;
                t.rounds++;
                t.inserts += ins;
            } else {
                bad += ins != 0;  // idle lanes and the slack behind an agent's candidates never insert
            }
        }
    }
    for (int l = 0; l < LANES; l++) {
        Lane &L = W[l];
        if (F != rh::PLAIN) rh::block_end(L.s.r[1], L.tm, L.s.tt);
        rh::block_rounds<K, F>(HostHeap{L.sb.col}, L.sb.r, L.sb.last, L.sb.q, wd[l], L.n - pb, L.tm, L.sb.tt, Told{&L.told, 0});
        rh::block_rounds<K, F>(HostHeap{L.sw.col}, L.sw.r, L.sw.last, wd[l], L.n - pb, L.tm, L.sw.tt, Told{&L.told, 0});
        wrap_bad += !same(L.s, L.sb, true) || !same(L.s, L.sw, false) || Told::overrun != 0;
        Told::overrun = 0;
    }
}

void run_wave(Lane (&W)[LANES], Tally &t) {
    int nmax = 0;
    bool wave_ties = false;
    for (Lane &L : W) {
        nmax = std::max(nmax, L.n);
        wave_ties |= L.on && L.has_tie;
    }
    long bad = 0, inv_bad = 0, mirror_bad = 0, wrap_bad = 0;
    // the fill, the track of the first K, make_heap in the form the wave takes
    unsigned int w[LANES][K / 2];
    bool any_first = false;
    for (int l = 0; l < LANES; l++) {
        Lane &L = W[l];
        for (int k = 0; k < K / 2; k++) w[l][k] = (uint32_t)L.E[2 * k] | ((uint32_t)L.E[2 * k + 1] << 16);
        std::memset(L.s.col, 0xff, sizeof(L.s.col));
        rh::fill_pairs<K>(HostHeap{L.s.col}, w[l]);
        any_first |= L.on && rh::any_tie(w[l], L.tm);
    }
    if (wave_ties && any_first)
        for (int l = 0; l < LANES; l++) {
            W[l].s.tt = rh::track_of(w[l], W[l].tm);
            if (!W[l].on) W[l].s.tt.tg = rh::NO_TIE;
        }
    bool heap_ties = false;
    for (Lane &L : W) heap_ties |= L.s.tt.tl();
    for (Lane &L : W) {
        const HostHeap H{L.s.col};
        if (L.on) {
            if (heap_ties) rh::make_heap<K, true>(H, L.tm);
            else rh::make_heap<K, false>(H, L.tm);
        }
        for (int j = 1; j < 8; j++) L.s.r[j] = H.get(j);
        L.s.last = H.get(K);
        rh::load_chain(H, L.s.q);  // where the kernel takes r[1..7] and last
        H.set(K, 0u);
        L.sb = L.s;
        L.sw = L.s;
        if (L.on) {
            auto cmp = [&](int a, int b) { return L.keys[a] < L.keys[b]; };
            L.ref.resize(K);
            std::iota(L.ref.begin(), L.ref.end(), 0);
            std::make_heap(L.ref.begin(), L.ref.end(), cmp);
            bad += heap_off(L) != 0;
        }
        mirror_bad += mirrors_off(L.s) != 0;
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
                // (the kernel asks any_tie of the block's four words first: a block with a tied candidate must pass that)
                inv_bad += rh::block_has_tie(wd[l], L.n - pb, L.tm) && !rh::any_tie(wd[l], L.tm);
                tracked |= wave_ties && L.s.tt.tl();
            }
            if (full) run_block<rh::TIES>(W, wd, pb, t, bad, inv_bad, mirror_bad, wrap_bad);
            else if (tracked) run_block<rh::CHECKED>(W, wd, pb, t, bad, inv_bad, mirror_bad, wrap_bad);
            else run_block<rh::PLAIN>(W, wd, pb, t, bad, inv_bad, mirror_bad, wrap_bad);
            t.ties_blocks += full;
            t.checked_blocks += !full && tracked;
        }
    }
    t.waves++;
    t.bad += bad != 0;
    t.inv_bad += inv_bad != 0;
    t.mirror_bad += mirror_bad != 0;
    t.wrap_bad += wrap_bad != 0;
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
    const int nw = argc > 1 ? std::atoi(argv[1]) : 40;
    long bad = 0;
    for (int kind = FREE; kind < NKINDS; kind++) {
        Tally t;
        for (int c = 0; c < nw; c++) {
            Lane W[LANES];
            const Format f = c % 2 ? LONG : STANDARD;  // the lane under test takes both formats in turn
            make_lane(W[0], kind == IDLE ? FREE : (Kind)kind, f);
            if (kind == IDLE) {  // one agent, every other lane idle
                for (int l = 1; l < LANES; l++) make_lane(W[l], IDLE, rnd() % 2 ? LONG : STANDARD);
            } else if (kind == FREE) {  // a wave without equal keys: never the equal-key form
                make_lane(W[1], FREE, rnd() % 2 ? LONG : STANDARD);
                make_lane(W[2], rnd() % 2 ? FREE : IDLE, f);
                make_lane(W[3], IDLE, STANDARD);
            } else {  // a lane without ties beside the tied one, a lane of any kind (either format), an idle or a short one
                make_lane(W[1], FREE, f);
                make_lane(W[2], (Kind)(rnd() % IDLE), rnd() % 2 ? LONG : STANDARD);
                make_lane(W[3], rnd() % 2 ? IDLE : FREE, STANDARD);
                if (W[3].on) { W[3].n = std::min(W[3].n, K + (int)(rnd() % 64)); W[3].keys.resize(W[3].n); W[3].E = ranks_of(W[3].keys, W[3].f.rsh); W[3].E.resize(LONG.nmax + 24, 0xffff); }
            }
            std::swap(W[0], W[rnd() % LANES]);  // the lane under test anywhere in the wave (the last one too)
            run_wave(W, t);
        }
        std::printf("%s waves %ld bad %ld inv_bad %ld mirror_bad %ld wrap_bad %ld rounds %ld inserts %ld via12 %ld via25 %ld via50 %ld via100 %ld "
                    "ties_blocks %ld checked_blocks %ld stepped_back %ld\n",
                    NAMES[kind], t.waves, t.bad, t.inv_bad, t.mirror_bad, t.wrap_bad, t.rounds, t.inserts, t.via[0], t.via[1], t.via[2], t.via[3],
                    t.ties_blocks, t.checked_blocks, t.stepped_back);
        bad += t.bad + t.inv_bad + t.mirror_bad + t.wrap_bad;
        for (int u = 0; u < 4; u++) bad += t.via[u] == 0;  // the pop's path never went through a mirrored slot: nothing was tested
        if (kind == FREE || kind == IDLE) bad += t.ties_blocks + t.checked_blocks;
    }
    std::printf("bad_access %ld\n", HostHeap::bad_access);
    return bad + HostHeap::bad_access != 0;
}
