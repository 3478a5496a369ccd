// k_knn_rank's candidate front end on the host: csrc/rank_cand.hpp (the decisions the kernel takes) run as the kernel runs
// them -- the block cull, a batch of 64 blocks at a time with the checkpoints counted as the kernel counts them, then the
// surviving blocks in index order through the per-road test -- against a plain loop over every road of the world with the
// checkpoint rule of the scan it replaces.  The two candidate lists must be equal element for element and no dropped block may
// hold a candidate.  One line per case:  name agents N bad B dropped_with_cand D blocks X survivors Y cands Z overflow O
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../gpudrive_lab_amd/csrc/rank_cand.hpp"

namespace rc = gd::rank_cand;

constexpr int K = 200;    // GD_MAP_OBS_K
constexpr int BLK = 16;   // GD_LIN_BLK
constexpr int NCP = 40;   // GD_RANK_NCP
constexpr int LSTN = 640; // the survivor list of the kernel (map_obs_rank.hip LSTN4)
const float INF = std::numeric_limits<float>::infinity();

struct World {
    std::vector<float> x, y;
    std::vector<float> cx, cy, rad;  // the circle around every BLK consecutive roads, as the engine builds it
    int R() const { return (int)x.size(); }
    void circles() {  // engine.cpp: centre of the bounding box, the largest distance from it, rounded up
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

struct Row {  // what k_knn_scan knows of an agent: the raw checkpoints
    float ex, ey;
    std::vector<unsigned int> first;
    std::vector<float> thr;
};

struct Tally { long agents = 0, bad = 0, dropped_with_cand = 0, blocks = 0, survivors = 0, cands = 0, overflow = 0; };

// the plain loop: every road, the scan's rule for the checkpoint in force
static std::vector<int> plain(const World &w, const Row &a) {
    std::vector<int> out;
    const int R = w.R();
    for (int r = 0; r < R; r++) {
        const int q = rc::cp_in_force(a.first.data(), (int)a.first.size(), r & ~(rc::CHUNK - 1));
        const float thr = q >= 0 ? a.thr[q] : INF;
        if (rc::is_candidate(r, K, R, w.x[r], w.y[r], a.ex, a.ey, thr)) out.push_back(r);
    }
    return out;
}

// the kernel's way.  `dropped` receives the blocks the cull dropped.
static std::vector<int> culled(const World &w, const Row &a, std::vector<int> &dropped, int &nsv_out, bool &list_ok) {
    const int R = w.R(), nblk = (R + BLK - 1) / BLK;
    // k_knn_scan's row: NCP entries, the running maximum of first[], (NO_CP, inf) behind the last one
    unsigned int cfirst[64];
    float cthr[64], creach[64];
    unsigned int run = 0u;
    for (int q = 0; q < 64; q++) {
        const bool have = q < (int)a.first.size() && q < NCP;
        if (have) run = rc::running_max(run, a.first[q]);
        cfirst[q] = have ? run : rc::NO_CP;
        cthr[q] = have ? a.thr[q] : INF;
        creach[q] = rc::block_reach(cthr[q]);
    }
    float tthr[NCP + 1];
    tthr[0] = INF;
    for (int q = 0; q < NCP; q++) tthr[q + 1] = cthr[q];
    std::vector<unsigned short> lst;
    for (int bb = 0; bb < nblk; bb += 64) {  // a batch: one block per lane
        const unsigned int base_lo = (unsigned int)rc::chunk_base_of_block(bb, BLK);
        const unsigned int base_hi = (unsigned int)rc::chunk_base_of_block(std::min(bb + 63, nblk - 1), BLK);
        int nlo = 0, nhi = 0;  // two ballots over the lanes that hold the row
        for (int q = 0; q < 64; q++) { nlo += cfirst[q] <= base_lo ? 1 : 0; nhi += cfirst[q] <= base_hi ? 1 : 0; }
        for (int lane = 0; lane < 64; lane++) {
            const int b = bb + lane;
            if (b >= nblk) break;
            const unsigned int base = (unsigned int)rc::chunk_base_of_block(b, BLK);
            int cnt = nlo;
            for (int q = nlo; q < nhi; q++) cnt += cfirst[q] <= base ? 1 : 0;
            if (cnt != rc::cp_count(cfirst, NCP, (int)base)) list_ok = false;  // the prefix argument
            const float reach = creach[(cnt - 1) & 63];
            if (rc::block_survives(b, BLK, K, w.cx[b], w.cy[b], w.rad[b], a.ex, a.ey, reach)) {
                if ((int)lst.size() >= LSTN || b >= 1024 || cnt > NCP) list_ok = false;
                lst.push_back((unsigned short)(b | cnt << 10));
            } else {
                dropped.push_back(b);
            }
        }
    }
    nsv_out = (int)lst.size();
    std::vector<int> out;
    for (unsigned short ent : lst) {  // index order; the kernel takes four blocks per pass, a road per lane
        const int b = ent & 1023, cnt = ent >> 10;
        for (int o = 0; o < BLK; o++) {
            const int r = b * BLK + o, rl = std::min(r, R - 1);
            if (rc::is_candidate(r, K, R, w.x[rl], w.y[rl], a.ex, a.ey, tthr[cnt])) out.push_back(r);
        }
    }
    return out;
}

static void check(const World &w, const Row &a, Tally &t) {
    std::vector<int> dropped;
    int nsv = 0;
    bool list_ok = true;
    const std::vector<int> want = plain(w, a), got = culled(w, a, dropped, nsv, list_ok);
    t.agents++;
    if (want != got || !list_ok) t.bad++;
    std::vector<char> has((w.R() + BLK - 1) / BLK, 0);
    for (int r : want) has[r / BLK] = 1;
    for (int b : dropped) t.dropped_with_cand += has[b];
    t.blocks += (long)has.size();
    t.survivors += nsv;
    t.cands += (long)want.size();
    t.overflow += (long)want.size() > 1272 ? 1 : 0;
}

// checkpoints as a previous selection leaves them: the K-th smallest squared distance over the roads before first[q], seen from
// where the agent was, widened by how far it moved since
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

static World walk_world(std::mt19937 &g, int R, float ox, float oy) {  // synth.make_scene's polylines
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

static std::vector<int> spaced_firsts(std::mt19937 &g, int R, int n) {  // ascending multiples of 32 from 192 on
    std::vector<int> f{(K / 32) * 32};
    std::uniform_int_distribution<int> gap(1, std::max(1, 2 * ((R + 31) / 32) / std::max(n, 1)));
    while ((int)f.size() < n) f.push_back(f.back() + 32 * gap(g));
    return f;
}

static void report(const char *name, const Tally &t) {
    std::printf("%s agents %ld bad %ld dropped_with_cand %ld blocks %ld survivors %ld cands %ld overflow %ld\n", name, t.agents, t.bad,
                t.dropped_with_cand, t.blocks, t.survivors, t.cands, t.overflow);
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 40;
    const int sizes[] = {K, K + 1, 207, 208, 209, 1271, 1272, 1273, 4096, 10000};
    std::mt19937 g(12345);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    long total_bad = 0;
    {   // random-walk polylines far from the origin, agents moving a little between selections
        Tally t;
        for (int R : sizes)
            for (int k = 0; k < reps; k++) {
                const float ox = 1000.f + 3000.f * u(g), oy = -500.f - 4000.f * u(g);
                const World w = walk_world(g, R, ox, oy);
                const float px = ox + 120.f * u(g) - 60.f, py = oy + 120.f * u(g) - 60.f;
                const float ex = px + 3.f * u(g) - 1.5f, ey = py + 3.f * u(g) - 1.5f;
                check(w, history_row(w, ex, ey, px, py, spaced_firsts(g, R, 1 + (int)(u(g) * 34.f))), t);
            }
        report("random_walk", t); total_bad += t.bad + t.dropped_with_cand;
    }
    {   // a checkpoint at every 32-road chunk from 192 on (as many as a row holds), then from a random later chunk on
        Tally t;
        for (int R : sizes)
            for (int k = 0; k < reps; k++) {
                const World w = walk_world(g, R, 2000.f, 3000.f);
                std::vector<int> f{192};
                const int skip = k == 0 ? 0 : (int)(u(g) * (float)(R / 32));
                for (int c = 7 + skip; (int)f.size() < NCP; c++) f.push_back(32 * c);
                const float px = 2000.f + 100.f * u(g) - 50.f, py = 3000.f + 100.f * u(g) - 50.f;
                check(w, history_row(w, px + 0.5f, py - 0.25f, px, py, f), t);
            }
        report("every_chunk", t); total_bad += t.bad + t.dropped_with_cand;
    }
    {   // thresholds that bound nothing, and tiny ones; first[] with repeats and out of order (the running maximum covers both)
        Tally t;
        for (int R : sizes)
            for (int k = 0; k < reps; k++) {
                const World w = walk_world(g, R, -3000.f, 1500.f);
                const float px = -3000.f + 100.f * u(g) - 50.f, py = 1500.f + 100.f * u(g) - 50.f;
                Row a = history_row(w, px, py, px, py, spaced_firsts(g, R, 2 + (int)(u(g) * 30.f)));
                for (size_t q = 0; q < a.thr.size(); q++) {
                    const float p = u(g);
                    if (p < 0.2f) a.thr[q] = INF;
                    else if (p < 0.4f) a.thr[q] = 1e-6f * u(g);
                    else if (p < 0.45f) a.thr[q] = 0.f;
                }
                for (size_t q = 1; q < a.first.size(); q++) {
                    const float p = u(g);
                    if (p < 0.15f) a.first[q] = a.first[q - 1];
                    else if (p < 0.25f && q >= 2) std::swap(a.first[q], a.first[q - 1]);
                }
                check(w, a, t);
            }
        report("inf_and_tiny", t); total_bad += t.bad + t.dropped_with_cand;
    }
    {   // an inward spiral: every road is closer than all before it, so under honest checkpoints every road is a candidate
        Tally t;
        for (int R : sizes) {
            World w;
            for (int r = 0; r < R; r++) {
                const float rho = 300.f * (1.f - (float)r / (float)R) + 1.f, ph = 0.05f * (float)r;
                w.x.push_back(5000.f + rho * std::cos(ph)); w.y.push_back(-7000.f + rho * std::sin(ph));
            }
            w.circles();
            std::vector<int> f{192};
            for (int c = 8; c * 32 < R && (int)f.size() < NCP; c += std::max(1, R / 32 / 38)) f.push_back(32 * c);
            const long before = t.cands;
            check(w, history_row(w, 5000.f, -7000.f, 5000.f, -7000.f, f), t);
            if (t.cands - before != R) { std::printf("spiral: %ld of %d roads are candidates\n", t.cands - before, R); total_bad++; }
            check(w, history_row(w, 5000.4f, -7000.3f, 5000.f, -7000.f, f), t);
        }
        report("spiral", t); total_bad += t.bad + t.dropped_with_cand;
    }
    {   // all roads at one point: the agent on it, near it, far from it
        Tally t;
        for (int R : sizes) {
            World w;
            w.x.assign(R, 4321.5f); w.y.assign(R, -1234.25f);
            w.circles();
            const std::vector<int> f = spaced_firsts(g, R, 12);
            check(w, history_row(w, 4321.5f, -1234.25f, 4321.5f, -1234.25f, f), t);
            check(w, history_row(w, 4322.5f, -1234.f, 4321.5f, -1234.25f, f), t);
            Row far = history_row(w, 9000.f, 9000.f, 4321.5f, -1234.25f, f);
            for (float &th : far.thr) th = 25.f;  // (a bound that no road meets)
            check(w, far, t);
        }
        report("one_point", t); total_bad += t.bad + t.dropped_with_cand;
    }
    {   // the agent exactly on a block's centre, on a road, and far outside the world, with thresholds at the block's own size
        Tally t;
        for (int R : sizes)
            for (int k = 0; k < reps; k++) {
                const World w = walk_world(g, R, 1500.f, -2500.f);
                const int nblk = (R + BLK - 1) / BLK, b = std::min(nblk - 1, (int)(u(g) * (float)nblk));
                const std::vector<int> f = spaced_firsts(g, R, 1 + (int)(u(g) * 30.f));
                Row a = history_row(w, w.cx[b], w.cy[b], w.cx[b], w.cy[b], f);
                check(w, a, t);
                for (float &th : a.thr) th = w.rad[b] * w.rad[b] * (0.5f + u(g));  // the boundary of the block's own circle
                check(w, a, t);
                const int r = std::min(R - 1, b * BLK + 3);
                check(w, history_row(w, w.x[r], w.y[r], w.x[r], w.y[r], f), t);
                Row out = history_row(w, 1500.f + 5000.f, -2500.f - 5000.f, 1500.f, -2500.f, f);
                check(w, out, t);
                for (float &th : out.thr) th = 400.f;
                check(w, out, t);
            }
        report("centre_and_far", t); total_bad += t.bad + t.dropped_with_cand;
    }
    return total_bad == 0 ? 0 : 1;
}
