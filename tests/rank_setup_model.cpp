// The set-up around k_knn_rank on the host (csrc/rank_cand.hpp): the checkpoint row of an agent that is bounded by its own
// checkpoints, as k_knn_scan's loop builds it against the way the 64 lanes of the ranking wave build it (cp_threshold per lane,
// the running maximum of the first roads as the wave's max-scan, nothing behind the last checkpoint) -- bit for bit; and the
// deal of worlds to k_knn_scan's workgroups (deal_block): a bijection that keeps every aligned group of 8, and how evenly it
// spreads scenes that repeat with a period over the eight XCD lists.  One line per case:
//   rows    name cases N bad B
//   deal    name grids N bad B
//   share   name cases N bad B                      (worlds tiled with periods 8 and 16: every XCD the even share of every scene)
//   load    name cases N bad B worst_milli M        (one scene 50 % dearer: the fullest list over the mean one, in thousandths)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../gpudrive_lab_amd/csrc/rank_cand.hpp"

namespace rc = gd::rank_cand;

constexpr int NCP = 40;  // GD_RANK_NCP
const float INF = std::numeric_limits<float>::infinity();

static unsigned int bits(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }

struct Row { unsigned int first[64]; float thr[64]; float t_last; };

// ---- k_knn_scan: one lane walks the agent's checkpoints; the entries behind the last one are never in force ----
static Row row_by_loop(const unsigned short *cr, const float *ct, int ncp, float move, float margin) {
    Row r;
    float t = 1.f;
    unsigned int fmax = 0u;
    for (int q = 0; q < 64; q++) { r.first[q] = rc::NO_CP; r.thr[q] = INF; }
    for (int q = 0; q < ncp; q++) {
        t = ct[q];
        fmax = rc::running_max(fmax, cr[q]);
        r.first[q] = (unsigned short)fmax;
        r.thr[q] = rc::cp_threshold(t, move, margin);
    }
    r.t_last = t;
    return r;
}

// ---- k_knn_rank: lane q holds entry q as recorded.  The wave's inclusive max-scan of non-negative values, step for step: shifts
// by 1, 2, 4, 8 inside each row of 16 lanes (a lane without a source takes 0), lane 15 of rows 0 and 2 into rows 1 and 3, lane 31
// into rows 2 and 3 ----
static void wave_incl_max_nonneg(int *v) {
    int s[64];
    for (int sh = 1; sh <= 8; sh <<= 1) {
        for (int l = 0; l < 64; l++) s[l] = (l & 15) >= sh ? v[l - sh] : 0;
        for (int l = 0; l < 64; l++) v[l] = std::max(v[l], s[l]);
    }
    for (int l = 0; l < 64; l++) s[l] = ((l >> 4) & 1) ? v[(l & ~15) - 1] : 0;  // row_bcast:15, rows 1 and 3
    for (int l = 0; l < 64; l++) v[l] = ((l >> 4) & 1) ? std::max(v[l], s[l]) : v[l];
    for (int l = 0; l < 64; l++) s[l] = l >= 32 ? v[31] : 0;                    // row_bcast:31, rows 2 and 3
    for (int l = 0; l < 64; l++) v[l] = l >= 32 ? std::max(v[l], s[l]) : v[l];
}
static Row row_by_lanes(const unsigned short *cr, const float *ct, int ncp, float move, float margin) {
    Row r;
    int v[64];
    float raw[64];
    for (int lane = 0; lane < 64; lane++) {  // rank_fetch: lanes below ncp load their entry, the others hold NO_CP / +inf
        const bool have = lane < ncp;
        raw[lane] = have ? ct[lane] : INF;
        v[lane] = have ? (int)cr[lane] : 0;
    }
    r.t_last = raw[ncp - 1];  // readlane(ncp - 1)
    wave_incl_max_nonneg(v);
    for (int lane = 0; lane < 64; lane++) {
        const bool have = lane < ncp;
        r.thr[lane] = have ? rc::cp_threshold(raw[lane], move, margin) : INF;
        r.first[lane] = have ? (unsigned int)v[lane] : rc::NO_CP;
    }
    return r;
}
static bool same(const Row &a, const Row &b) {
    for (int q = 0; q < 64; q++)
        if (a.first[q] != b.first[q] || bits(a.thr[q]) != bits(b.thr[q])) return false;
    return bits(a.t_last) == bits(b.t_last);
}

static int rows_cases() {
    const int ncps[] = {1, 2, 39, 40};
    const float moves[] = {0.f, 5.999f, rc::CP_MOVE_MAX};
    const float margins[] = {1.00001f, 1.0000143f, 1.37f};
    const float denormal = std::numeric_limits<float>::denorm_min() * 37.f;
    const float specials[] = {0.f, denormal, 1e30f, INF, std::numeric_limits<float>::quiet_NaN(), -4.f, 153.25f};
    // first roads: increasing; non-monotone; with the 16-bit image of NO_CP (cp_road holds 16 bits) in the middle and at the end
    std::vector<std::vector<unsigned short>> firsts;
    {
        std::vector<unsigned short> inc(NCP), zig(NCP), nocp(NCP), flat(NCP, 192), big(NCP);
        for (int q = 0; q < NCP; q++) {
            inc[q] = (unsigned short)(192 + 32 * q * (q + 3));
            zig[q] = (unsigned short)(192 + 32 * ((q * 29) % 41));
            nocp[q] = (q == 17 || q == 38 || q == 39) ? (unsigned short)rc::NO_CP : inc[q];
            big[q] = (unsigned short)(65535 - 32 * ((q * 7) % 40));
        }
        nocp[0] = 0;
        firsts = {inc, zig, nocp, flat, big};
    }
    long cases = 0, bad = 0;
    for (int ncp : ncps)
        for (float move : moves)
            for (float margin : margins)
                for (const auto &cr : firsts)
                    for (float sp : specials)
                        for (int at : {0, 1, ncp / 2, ncp - 2, ncp - 1}) {
                            if (at < 0 || at >= ncp) continue;
                            float ct[NCP];
                            for (int q = 0; q < NCP; q++) ct[q] = 2500.f / (1.f + 0.37f * (float)q) + 0.013f * (float)(q * q);
                            ct[at] = sp;
                            const Row a = row_by_loop(cr.data(), ct, ncp, move, margin), b = row_by_lanes(cr.data(), ct, ncp, move, margin);
                            cases++;
                            bad += same(a, b) ? 0 : 1;
                            // (the rule itself: an unusable key bounds nothing, a usable one is at least the key)
                            const float thr = a.thr[at];
                            if (!(sp >= 0.f) && thr != INF) bad++;
                            if (sp >= 0.f && !(thr >= sp)) bad++;
                        }
    std::printf("rows own_checkpoints cases %ld bad %ld\n", cases, bad);
    return bad ? 1 : 0;
}

// ---- the deal ----
static std::vector<int> grids() {
    std::vector<int> g;
    for (int n = 1; n <= 130; n++) g.push_back(n);
    for (int n : {1000, 1024, 1025, 4096}) g.push_back(n);
    return g;
}
static int deal_cases() {
    long bad = 0;
    const std::vector<int> gs = grids();
    for (int grid : gs) {
        std::vector<int> hit((size_t)grid, 0);
        for (int b = 0; b < grid; b++) {
            const int w = rc::deal_block(b, grid);
            if (w < 0 || w >= grid) { bad++; continue; }
            hit[(size_t)w]++;
            if ((w >> 3) != (b >> 3)) bad++;                      // an aligned group of 8 onto itself
            if ((b | 7) >= grid && w != b) bad++;                 // the identity on a last partial group
            if (rc::deal_list(w, grid) != (b & 7)) bad++;         // the list of a world: the inverse deal
        }
        for (int w = 0; w < grid; w++) bad += hit[(size_t)w] == 1 ? 0 : 1;  // a bijection
    }
    std::printf("deal bijection_groups grids %zu bad %ld\n", gs.size(), bad);
    return bad ? 1 : 0;
}
// worlds on XCD list x: those deal_block gives the b with b % 8 == x (deal_list: the same from the world's side).  load[x][scene]
static std::vector<std::vector<int>> shares(int grid, int period, bool dealt) {
    std::vector<std::vector<int>> n(8, std::vector<int>((size_t)period, 0));
    for (int b = 0; b < grid; b++) n[(size_t)(b & 7)][(size_t)((dealt ? rc::deal_block(b, grid) : b) % period)]++;
    return n;
}
static int share_cases() {
    long cases = 0, bad = 0;
    for (int grid : {1024, 4096})
        for (int period : {8, 16}) {
            const auto n = shares(grid, period, true);
            for (int x = 0; x < 8; x++)
                for (int s = 0; s < period; s++) {
                    cases++;
                    bad += n[(size_t)x][(size_t)s] == grid / 8 / period ? 0 : 1;
                }
        }
    std::printf("share even_per_scene cases %ld bad %ld\n", cases, bad);
    return bad ? 1 : 0;
}
// the fullest list over the mean one, scene `dear` costing 1.5 and the others 1
static double worst_load(int grid, int period, bool dealt) {
    const auto n = shares(grid, period, dealt);
    double worst = 0.0;
    for (int dear = 0; dear < period; dear++) {
        double load[8], sum = 0.0, mx = 0.0;
        for (int x = 0; x < 8; x++) {
            load[x] = 0.0;
            for (int s = 0; s < period; s++) load[x] += (s == dear ? 1.5 : 1.0) * n[(size_t)x][(size_t)s];
            sum += load[x];
            mx = std::max(mx, load[x]);
        }
        worst = std::max(worst, mx / (sum / 8.0));
    }
    return worst;
}
static int load_cases() {
    long cases = 0, bad = 0;
    double worst = 0.0, worst_identity = 0.0;
    for (int grid : {1024, 4096})
        for (int period = 1; period <= 128; period++) {
            const double r = worst_load(grid, period, true);
            cases++;
            bad += r <= 1.08 ? 0 : 1;
            worst = std::max(worst, r);
            worst_identity = std::max(worst_identity, worst_load(grid, period, false));
        }
    std::printf("load dealt cases %ld bad %ld worst_milli %ld\n", cases, bad, std::lround(worst * 1000.0));
    // (what the deal is for: workgroup b on world b puts every copy of the dear scene on one list)
    std::printf("load identity cases %ld bad %d worst_milli %ld\n", cases, worst_identity > 1.4 ? 0 : 1, std::lround(worst_identity * 1000.0));
    return (bad || !(worst_identity > 1.4)) ? 1 : 0;
}

int main() {
    int rc_ = 0;
    rc_ |= rows_cases();
    rc_ |= deal_cases();
    rc_ |= share_cases();
    rc_ |= load_cases();
    return rc_;
}
