// k_knn_rank's table of checkpoints per 32-road chunk on the host: csrc/rank_cand.hpp cp_table (the rule) and the way the kernel
// builds it -- lane q scatters q + 1 with a max, every lane scans consecutive entries, a max-scan across the lanes carries the
// rest -- against cp_count and cp_in_force + 1 for every chunk of the world; then the cull and the ordered scan as the kernel
// runs them with that table (one read per block; passes of four listed blocks, all but the last without a clamp) against the
// cull that counts the checkpoints per block with cp_count: survivor lists and candidate lists equal element for element, no
// dropped block with a candidate of the plain loop over every road.  One line per case:
//   table   name rows N bad B                                   (bad: rows with any chunk that differs)
//   lists   name agents N bad B dropped_with_cand D survivors Y cands Z unclamped_beyond_world U
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../gpudrive_lab_amd/csrc/rank_cand.hpp"

namespace rc = gd::rank_cand;

constexpr int K = 200;    // GD_MAP_OBS_K
constexpr int BLK = 16;   // GD_LIN_BLK
constexpr int NCP = 40;   // GD_RANK_NCP
constexpr int BPP = 64 / BLK;
const float INF = std::numeric_limits<float>::infinity();

// ---- the row as k_knn_scan stores it and as k_knn_rank's lanes hold it: 64 entries, the running maximum, NO_CP behind the last ----
struct Lanes { unsigned int cfirst[64]; float cthr[64], creach[64]; };
static Lanes lanes_of(const std::vector<unsigned int> &first, const std::vector<float> &thr) {
    Lanes l;
    unsigned int run = 0u;
    for (int q = 0; q < 64; q++) {
        const bool have = q < (int)first.size() && q < NCP;
        if (have) run = rc::running_max(run, first[q]);
        l.cfirst[q] = have ? run : rc::NO_CP;
        l.cthr[q] = have ? thr[q] : INF;
        l.creach[q] = rc::block_reach(l.cthr[q]);
    }
    return l;
}

// ---- the table the way the kernel builds it ----
static std::vector<unsigned int> kernel_table(const Lanes &l, int R) {
    const int nch = rc::chunks_of(R), epl = (nch + 63) >> 6;
    std::vector<unsigned int> tmax((size_t)64 * epl, 0u), out((size_t)64 * epl, 0u);
    for (int lane = 0; lane < NCP; lane++)  // scatter: an LDS max per lane
        if (rc::cp_table_takes(l.cfirst[lane], nch)) {
            unsigned int &e = tmax[rc::cp_table_chunk(l.cfirst[lane])];
            e = std::max(e, rc::cp_table_entry(lane));
        }
    unsigned int last[64], incl[64];
    for (int lane = 0; lane < 64; lane++) {  // each lane on its consecutive entries
        unsigned int run = 0u;
        for (int u = 0; u < epl; u++) { run = std::max(run, tmax[(size_t)lane * epl + u]); out[(size_t)lane * epl + u] = run; }
        last[lane] = run;
    }
    for (int lane = 0; lane < 64; lane++) incl[lane] = std::max(last[lane], lane ? incl[lane - 1] : 0u);  // the max-scan across lanes
    for (int lane = 1; lane < 64; lane++)
        for (int u = 0; u < epl; u++) out[(size_t)lane * epl + u] = std::max(out[(size_t)lane * epl + u], incl[lane - 1]);
    out.resize(nch);
    return out;
}

static long table_bad(const std::vector<unsigned int> &first, int R) {
    const Lanes l = lanes_of(first, std::vector<float>(first.size(), 1.f));
    const int nch = rc::chunks_of(R);
    std::vector<unsigned int> rule((size_t)nch);
    rc::cp_table(rule.data(), nch, l.cfirst, NCP);
    const std::vector<unsigned int> kern = kernel_table(l, R);
    const int n = std::min((int)first.size(), NCP);
    for (int c = 0; c < nch; c++) {
        const int base = c * rc::CHUNK;
        const int want = rc::cp_count(l.cfirst, NCP, base);
        if (want != rc::cp_in_force(first.data(), n, base) + 1) return 1;
        if ((int)rule[c] != want || (int)kern[c] != want || want > NCP) return 1;
    }
    return 0;
}

// ---- worlds and rows: the generators of tests/rank_cand_model.cpp ----
struct World {
    std::vector<float> x, y, cx, cy, rad;
    int R() const { return (int)x.size(); }
    void circles() {
        const int nr = R();
        for (int lo = 0; lo < nr; lo += BLK) {
            const int hi = std::min(nr, lo + BLK);
            float lx = INF, ly = INF, hx = -INF, hy = -INF;
            for (int r = lo; r < hi; r++) { lx = std::min(lx, x[r]); hx = std::max(hx, x[r]); ly = std::min(ly, y[r]); hy = std::max(hy, y[r]); }
            const float mx = 0.5f * (lx + hx), my = 0.5f * (ly + hy);
            float rd = 0.f;
            for (int r = lo; r < hi; r++) rd = std::max(rd, std::sqrt((x[r] - mx) * (x[r] - mx) + (y[r] - my) * (y[r] - my)));
            cx.push_back(mx); cy.push_back(my); rad.push_back(rd * 1.0001f + 1e-3f);
        }
    }
};
struct Row { float ex, ey; std::vector<unsigned int> first; std::vector<float> thr; };

static Row history_row(const World &w, float ex, float ey, float px, float py, const std::vector<int> &firsts) {
    Row a{ex, ey, {}, {}};
    const float move = std::sqrt((ex - px) * (ex - px) + (ey - py) * (ey - py));
    std::vector<float> d2;
    for (int f : firsts) {
        d2.clear();
        for (int r = 0; r < std::min(f, w.R()); r++) d2.push_back((w.x[r] - px) * (w.x[r] - px) + (w.y[r] - py) * (w.y[r] - py));
        float T = INF;
        if ((int)d2.size() >= K) { std::nth_element(d2.begin(), d2.begin() + (K - 1), d2.end()); T = d2[K - 1]; }
        const float reach = std::sqrt(T) * 1.0001f + move * 1.0001f + 1e-3f;
        float thr = reach * reach * 1.0001f * 1.00001f;
        if (!(thr >= 0.f)) thr = INF;
        a.first.push_back((unsigned int)f);
        a.thr.push_back(thr);
    }
    return a;
}
static World walk_world(std::mt19937 &g, int R, float ox, float oy) {
    World w;
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::normal_distribution<float> nrm(0.f, 0.1f);
    while (w.R() < R) {
        float x = ox + (u(g) * 160.f - 80.f), y = oy + (u(g) * 160.f - 80.f), th = u(g) * 6.2831853f;
        for (int k = 0; k < 128 && w.R() < R; k++) {
            th += nrm(g);
            const float step = 0.5f + 4.5f * u(g);
            x += step * std::cos(th);
            y += step * std::sin(th);
            w.x.push_back(x); w.y.push_back(y);
        }
    }
    w.circles();
    return w;
}
static std::vector<int> spaced_firsts(std::mt19937 &g, int R, int n) {
    std::vector<int> f{(K / 32) * 32};
    std::uniform_int_distribution<int> gap(1, std::max(1, 2 * ((R + 31) / 32) / std::max(n, 1)));
    while ((int)f.size() < n) f.push_back(f.back() + 32 * gap(g));
    return f;
}

// ---- cull + scan ----
struct Lists { std::vector<unsigned short> lst; std::vector<int> cands, dropped; long beyond = 0; };

static std::vector<int> plain(const World &w, const Row &a) {
    std::vector<int> out;
    const int R = w.R();
    for (int r = 0; r < R; r++) {
        const int q = rc::cp_in_force(a.first.data(), std::min((int)a.first.size(), NCP), r & ~(rc::CHUNK - 1));
        if (rc::is_candidate(r, K, R, w.x[r], w.y[r], a.ex, a.ey, q >= 0 ? a.thr[q] : INF)) out.push_back(r);
    }
    return out;
}

// by_table: the count of a block is one read of the kernel's table; else cp_count per block
static Lists cull_scan(const World &w, const Row &a, bool by_table) {
    const int R = w.R(), nblk = (R + BLK - 1) / BLK;
    const Lanes l = lanes_of(a.first, a.thr);
    float tthr[NCP + 1];
    tthr[0] = INF;
    for (int q = 0; q < NCP; q++) tthr[q + 1] = l.cthr[q];
    const std::vector<unsigned int> tab = kernel_table(l, R);
    Lists out;
    for (int b = 0; b < nblk; b++) {
        const int base = rc::chunk_base_of_block(b, BLK);
        const int cnt = by_table ? (int)tab[base / rc::CHUNK] : rc::cp_count(l.cfirst, NCP, base);
        if (rc::block_survives(b, BLK, K, w.cx[b], w.cy[b], w.rad[b], a.ex, a.ey, l.creach[(cnt - 1) & 63]))
            out.lst.push_back((unsigned short)(b | cnt << 10));
        else
            out.dropped.push_back(b);
    }
    const int nsv = (int)out.lst.size(), np = (nsv + BPP - 1) / BPP, nfast = np - 1;
    for (int p = 0; p < np; p++)
        for (int lane = 0; lane < 64; lane++) {
            const int e = p * BPP + lane / BLK, o = lane % BLK;
            if (by_table && p < nfast) {  // the main loop's passes: no test of e, no clamp of the road
                const int r = (out.lst[e] & 1023) * BLK + o;
                if (r >= R) { out.beyond++; continue; }
                if (rc::is_candidate(r, K, R, w.x[r], w.y[r], a.ex, a.ey, tthr[out.lst[e] >> 10])) out.cands.push_back(r);
            } else {
                const bool on = e < nsv;
                const int r = on ? (out.lst[e] & 1023) * BLK + o : R, rl = std::min(r, R - 1);
                if (rc::is_candidate(r, K, R, w.x[rl], w.y[rl], a.ex, a.ey, tthr[on ? std::min(out.lst[e] >> 10, NCP) : 0])) out.cands.push_back(r);
            }
        }
    return out;
}

struct Tally { long agents = 0, bad = 0, dropped_with_cand = 0, survivors = 0, cands = 0, beyond = 0; };
static void check(const World &w, const Row &a, Tally &t) {
    const Lists got = cull_scan(w, a, true), want = cull_scan(w, a, false);
    const std::vector<int> all = plain(w, a);
    t.agents++;
    if (got.lst != want.lst || got.cands != want.cands || got.cands != all) t.bad++;
    std::vector<char> has((w.R() + BLK - 1) / BLK, 0);
    for (int r : all) has[r / BLK] = 1;
    for (int b : got.dropped) t.dropped_with_cand += has[b];
    t.survivors += (long)got.lst.size();
    t.cands += (long)got.cands.size();
    t.beyond += got.beyond;
}
static long report(const char *name, const Tally &t) {
    std::printf("lists %s agents %ld bad %ld dropped_with_cand %ld survivors %ld cands %ld unclamped_beyond_world %ld\n", name, t.agents, t.bad,
                t.dropped_with_cand, t.survivors, t.cands, t.beyond);
    return t.bad + t.dropped_with_cand + t.beyond;
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 20;
    const int sizes[] = {200, 201, 207, 208, 209, 1024, 1025, 1271, 1272, 1273, 4096, 10000};
    std::mt19937 g(24680);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    long total_bad = 0;
    // ---- the table, for every chunk of the world ----
    struct { const char *name; long rows, bad; } tt[8] = {{"none", 0, 0}, {"all_forty", 0, 0}, {"repeats", 0, 0}, {"one_chunk", 0, 0},
                                                          {"first_zero", 0, 0}, {"at_and_beyond_end", 0, 0}, {"out_of_order", 0, 0}, {"any_value", 0, 0}};
    auto table_case = [&](int k, const std::vector<unsigned int> &first, int R) { tt[k].rows++; tt[k].bad += table_bad(first, R); };
    for (int R : sizes) {
        const int nch = rc::chunks_of(R);
        table_case(0, {}, R);
        table_case(0, std::vector<unsigned int>(NCP, rc::NO_CP), R);
        for (int k = 0; k < reps; k++) {
            std::vector<unsigned int> f;
            {   // all 40 in use, ascending, from a random chunk on with random gaps
                unsigned int c = (unsigned int)(u(g) * 8.f);
                for (int q = 0; q < NCP; q++) { f.push_back(32u * c); c += 1u + (unsigned int)(u(g) * (float)(2 * nch / NCP + 1)); }
                table_case(1, f, R);
            }
            {   // first roads repeated
                f.clear();
                unsigned int c = 6u;
                const int n = 2 + (int)(u(g) * 38.f);
                for (int q = 0; q < n; q++) { f.push_back(32u * c); if (u(g) < 0.5f) c += (unsigned int)(u(g) * 6.f); }
                table_case(2, f, R);
            }
            {   // several checkpoints starting in one chunk, here and there
                f.clear();
                unsigned int c = (unsigned int)(u(g) * (float)nch);
                for (int q = 0; q < NCP; q++) { f.push_back(32u * c); if (q % 7 == 6) c += 1u + (unsigned int)(u(g) * 3.f); }
                table_case(3, f, R);
            }
            {   // a first road of 0
                f.assign(1, 0u);
                const int n = (int)(u(g) * 39.f);
                for (int q = 0; q < n; q++) f.push_back(f.back() + 32u * (unsigned int)(u(g) * 4.f));
                table_case(4, f, R);
            }
            {   // first roads at the last chunk, at the world's end and beyond
                f.clear();
                const unsigned int lastc = (unsigned int)(nch - 1);
                f.push_back(32u * (lastc > 2u ? lastc - 2u : 0u));
                f.push_back(32u * lastc);
                f.push_back(32u * lastc);
                f.push_back(32u * (lastc + 1u));
                f.push_back(32u * (lastc + 1u + (unsigned int)(u(g) * 50.f)));
                f.push_back(65504u);
                f.push_back(0xffffffe0u);
                table_case(5, f, R);
            }
            {   // out of order: the running maximum makes the row non-decreasing
                f.clear();
                const int n = 1 + (int)(u(g) * 40.f);
                for (int q = 0; q < n; q++) f.push_back(32u * (unsigned int)(u(g) * (float)(nch + 4)));
                table_case(6, f, R);
            }
            {   // not multiples of 32 (the engine writes none: the rule holds all the same)
                f.clear();
                const int n = 1 + (int)(u(g) * 40.f);
                for (int q = 0; q < n; q++) f.push_back((unsigned int)(u(g) * (float)(R + 100)));
                std::sort(f.begin(), f.end());
                table_case(7, f, R);
            }
        }
    }
    for (const auto &t : tt) {
        std::printf("table %s rows %ld bad %ld\n", t.name, t.rows, t.bad);
        total_bad += t.bad;
    }
    // ---- survivor and candidate lists ----
    {
        Tally t;
        for (int R : sizes)
            for (int k = 0; k < reps; k++) {
                const float ox = 1000.f + 3000.f * u(g), oy = -500.f - 4000.f * u(g);
                const World w = walk_world(g, R, ox, oy);
                const float px = ox + 120.f * u(g) - 60.f, py = oy + 120.f * u(g) - 60.f;
                const float ex = px + 3.f * u(g) - 1.5f, ey = py + 3.f * u(g) - 1.5f;
                Row a = history_row(w, ex, ey, px, py, spaced_firsts(g, R, 1 + (int)(u(g) * 39.f)));
                check(w, a, t);
                for (size_t q = 1; q < a.first.size(); q++) {  // repeats and swaps
                    const float p = u(g);
                    if (p < 0.15f) a.first[q] = a.first[q - 1];
                    else if (p < 0.25f && q >= 2) std::swap(a.first[q], a.first[q - 1]);
                }
                check(w, a, t);
            }
        total_bad += report("random_walk", t);
    }
    {
        Tally t;
        for (int R : sizes) {
            World w;
            for (int r = 0; r < R; r++) {
                const float rho = 300.f * (1.f - (float)r / (float)R) + 1.f, ph = 0.05f * (float)r;
                w.x.push_back(5000.f + rho * std::cos(ph)); w.y.push_back(-7000.f + rho * std::sin(ph));
            }
            w.circles();
            std::vector<int> f{192};
            for (int c = 7; c * 32 < R + 64 && (int)f.size() < NCP; c++) f.push_back(32 * c);  // a checkpoint in every chunk until the 40 are used
            check(w, history_row(w, 5000.f, -7000.f, 5000.f, -7000.f, f), t);
            check(w, history_row(w, 5000.4f, -7000.3f, 5000.f, -7000.f, f), t);
        }
        total_bad += report("spiral", t);
    }
    {
        Tally t;
        for (int R : sizes) {
            World w;
            w.x.assign(R, 4321.5f); w.y.assign(R, -1234.25f);
            w.circles();
            const std::vector<int> f = spaced_firsts(g, R, 12);
            check(w, history_row(w, 4321.5f, -1234.25f, 4321.5f, -1234.25f, f), t);
            check(w, history_row(w, 4322.5f, -1234.f, 4321.5f, -1234.25f, f), t);
            Row far = history_row(w, 9000.f, 9000.f, 4321.5f, -1234.25f, f);
            for (float &th : far.thr) th = 25.f;
            check(w, far, t);
        }
        total_bad += report("one_point", t);
    }
    return total_bad == 0 ? 0 : 1;
}
