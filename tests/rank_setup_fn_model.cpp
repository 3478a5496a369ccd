// The per-lane decision of the rank path's set-up (csrc/rank_setup.hpp decide: what k_world_step and k_knn_scan run) against the
// expressions of the kernel it was taken out of, restated below as that kernel had them: the far test, the choice of the
// checkpoint set, donor borrowing, eligibility and bypass, `move`, `margin`, and the 16-byte record of an agent bounded by its
// own checkpoints -- bit for bit, over seeded headers and poses.  One line per family of cases:
//   decide  name cases N bad B far F fallback L afresh S own O row R
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../gpudrive_lab_amd/csrc/rank_setup.hpp"

namespace rs = gd::rank_setup;

struct F4 { float x, y, z, w; };
const float INF = std::numeric_limits<float>::infinity();
constexpr int K = 200;                      // GD_MAP_OBS_K
constexpr float CP_MOVE_MAX = 6.f;          // rank_cand.hpp
constexpr int REC_ROW = 1 << 16;            // GD_RK_REC_ROW

static unsigned int bits(float f) { unsigned int u; std::memcpy(&u, &f, 4); return u; }
static float as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
static int as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }

struct Inputs {
    int lane;
    float ex, ey, iw, iz;
    F4 h0, h1, bb, hdr[64];
    int R, min_roads, max_roads, streak, selections, grp;
    float radius;
    bool scan_rows;
};

// What the former kernel left for one live lane: rk_n, rk_ticket, whether the fallback flag was raised, the lane's ncp (-1: to be
// bounded afresh), whether it got no row, the source of its checkpoints, and the record it wrote (own checkpoints or a row)
struct Former {
    int state, reason, fallback, ncp, own, set, src_lane, rec_written;
    float rec[3];
    float move, margin;
};

static Former former_kernel(const Inputs &in) {
    Former o{};
    const float ex = in.ex, ey = in.ey;
    const F4 h0 = in.h0, h1 = in.h1;
    const int R = in.R, lane = in.lane;
    int ncp = 0;
    bool own_cp = false;
    o.src_lane = lane;
    const F4 bb = in.bb;
    const float ddx = fmaxf(fmaxf(bb.x - ex, ex - bb.z), 0.f), ddy = fmaxf(fmaxf(bb.y - ey, ey - bb.w), 0.f);
    const float far = in.radius * 1.01f + 1.f;
    int state = 1, reason = -1;
    if (R >= K && ddx * ddx + ddy * ddy > far * far) {
        state = rs::RK_FAR;
    } else {
        const int n0 = as_int(h0.z), n1 = as_int(h1.z);
        const float m0 = n0 > 0 ? sqrtf((ex - h0.x) * (ex - h0.x) + (ey - h0.y) * (ey - h0.y)) : INF;
        const float m1 = n1 > 0 ? sqrtf((ex - h1.x) * (ex - h1.x) + (ey - h1.y) * (ey - h1.y)) : INF;
        int set = m1 < m0 ? 1 : 0;
        float move = set ? m1 : m0;
        int n_cp = set ? n1 : n0;
        int src = lane;
        if (move > CP_MOVE_MAX) {
            float best = move;
            int donor = -1;
            for (int j = 0; j < 64; j++) {
                const F4 hj = in.hdr[j];
                const float dj = as_int(hj.z) > 0 ? sqrtf((ex - hj.x) * (ex - hj.x) + (ey - hj.y) * (ey - hj.y)) : INF;
                if (dj < best) { best = dj; donor = j; }
            }
            if (donor >= 0) {
                move = best;
                set = 0;
                n_cp = as_int(in.hdr[donor].z);
                src = donor;
            }
        }
        const bool eligible = R >= K && R >= in.min_roads && R <= in.max_roads;
        const bool bypass = eligible && in.streak >= 3 && ((in.selections + in.grp) & 63) != 0;
        const float iw = in.iw, iz = in.iz;
        const float z2 = iz * iz;
        const float det = (1.f - 2.f * z2) * (1.f - 2.f * z2) + 4.f * z2 * (iw * iw);
        const float margin = 1.00001f / fminf(det, 1.f);
        o.move = move; o.margin = margin; o.set = set; o.src_lane = src;
        if (!eligible || bypass) {
            state = 0;
            ncp = 0;
            reason = bypass ? -5 : -2;
            o.fallback = 1;
        } else if (n_cp <= 0 || move > CP_MOVE_MAX) {
            ncp = -1;
        } else if (src == lane && !in.scan_rows) {
            ncp = n_cp;
            own_cp = true;
            o.rec_written = 1;
            o.rec[0] = move; o.rec[1] = margin; o.rec[2] = as_float(n_cp | set << 8);
        } else {
            ncp = n_cp;
            o.rec_written = 2;  // (move, the last K-th key of the copied row, n_cp | REC_ROW)
            o.rec[0] = move; o.rec[1] = 0.f; o.rec[2] = as_float(n_cp | REC_ROW);
        }
    }
    if (state == rs::RK_FAR) ncp = 0;
    o.state = state; o.reason = reason; o.ncp = ncp; o.own = own_cp ? 1 : 0;
    return o;
}

// the same facts from the header's decision, put together as rank_setup::run does
static Former from_decision(const Inputs &in, int *kind) {
    const rs::Decision d = rs::decide(in.lane, in.ex, in.ey, in.iw, in.iz, in.h0, in.h1, in.bb, in.hdr, in.R, K, in.radius,
                                      in.min_roads, in.max_roads, in.streak, in.selections, in.grp, in.scan_rows);
    Former o{};
    *kind = d.kind;
    o.state = d.state; o.reason = d.reason;
    o.src_lane = d.donor >= 0 ? d.donor : in.lane;
    o.move = d.move; o.margin = d.margin; o.set = d.set;
    switch (d.kind) {
    case rs::FAR: o.src_lane = in.lane; break;
    case rs::FALLBACK: o.fallback = 1; break;
    case rs::AFRESH: o.ncp = -1; break;
    case rs::OWN:
        o.ncp = d.n_cp; o.own = 1; o.rec_written = 1;
        o.rec[0] = d.move; o.rec[1] = d.margin; o.rec[2] = as_float(rs::own_record_bits(d));
        break;
    default:
        o.ncp = d.n_cp; o.rec_written = 2;
        o.rec[0] = d.move; o.rec[1] = 0.f; o.rec[2] = as_float(d.n_cp | REC_ROW);
        break;
    }
    return o;
}

static bool same(const Former &a, const Former &b) {
    if (a.state != b.state || a.reason != b.reason || a.fallback != b.fallback || a.ncp != b.ncp || a.own != b.own ||
        a.rec_written != b.rec_written)
        return false;
    if (a.state == rs::RK_FAR) return true;  // (nothing else is used of a far agent)
    if (a.set != b.set || a.src_lane != b.src_lane || bits(a.move) != bits(b.move) || bits(a.margin) != bits(b.margin)) return false;
    for (int k = 0; k < 3; k++)
        if (bits(a.rec[k]) != bits(b.rec[k])) return false;
    return true;
}

// A header recorded `dist` metres from (ex, ey) in a random direction, with n checkpoints
static F4 header_at(std::mt19937 &g, float ex, float ey, float dist, int n) {
    const float th = std::uniform_real_distribution<float>(0.f, 6.2831853f)(g);
    return F4{ex + dist * cosf(th), ey + dist * sinf(th), as_float(n), 0.f};
}

static int run_family(const char *name, unsigned int seed, int cases, int family) {
    std::mt19937 g(seed);
    auto uf = [&](float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(g); };
    auto ui = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g); };
    const float dists[] = {0.f, 0.3f, 2.5f, 5.999f, 6.f, 6.0001f, 9.f, 40.f, 900.f};
    const int counts[] = {0, -1, 1, 2, 17, 39, 40};
    const int roads[] = {100, 199, 200, 300, 1535, 1536, 5000, 10000, 10001};
    int bad = 0, kinds[5] = {0, 0, 0, 0, 0};
    for (int c = 0; c < cases; c++) {
        Inputs in{};
        in.lane = ui(0, 63);
        in.ex = uf(-400.f, 400.f); in.ey = uf(-400.f, 400.f);
        const float yaw = uf(-3.2f, 3.2f), scale = family == 3 ? uf(0.9f, 1.1f) : 1.f;  // (a stored quaternion is a unit one only up to rounding)
        in.iw = cosf(yaw / 2.f) * scale; in.iz = sinf(yaw / 2.f) * scale;
        in.radius = family == 0 ? 50.f : uf(10.f, 120.f);
        // the world's roads: around the agent as a rule; family 1 puts the box to one side, at distances around `far`
        float cx = in.ex + uf(-30.f, 30.f), cy = in.ey + uf(-30.f, 30.f), hx = uf(1.f, 200.f), hy = uf(1.f, 200.f);
        if (family == 1) {
            const float far = in.radius * 1.01f + 1.f, gap = far * uf(0.5f, 1.5f), th = uf(0.f, 6.2831853f);
            cx = in.ex + (gap + hx) * cosf(th); cy = in.ey + (gap + hy) * sinf(th);
        }
        in.bb = F4{cx - hx, cy - hy, cx + hx, cy + hy};
        in.R = roads[ui(0, 8)];
        in.min_roads = ui(0, 1) ? 200 : 1536;
        in.max_roads = ui(0, 3) ? 10000 : 4000;
        in.streak = ui(0, 3);
        in.selections = ui(0, 1 << 20);
        in.grp = ui(0, 1 << 16);
        in.scan_rows = family == 4 || (family != 0 && ui(0, 7) == 0);
        in.h0 = header_at(g, in.ex, in.ey, dists[ui(0, 8)], counts[ui(0, 6)]);
        in.h1 = header_at(g, in.ex, in.ey, dists[ui(0, 8)], counts[ui(0, 6)]);
        if (family == 0) {  // an ordinary step: a few centimetres from the previous selection
            in.h0 = header_at(g, in.ex, in.ey, uf(0.f, 3.f), ui(1, 40));
            in.h1 = header_at(g, in.ex, in.ey, uf(0.f, 60.f), ui(1, 40));
            in.R = 4096; in.streak = 0; in.max_roads = 10000;
        }
        for (int j = 0; j < 64; j++) {
            // neighbours: mostly far away or without checkpoints, rarely one within reach (family 2: in two cases of three)
            const bool near = ui(0, family == 2 ? 60 : 400) == 0;
            in.hdr[j] = header_at(g, in.ex, in.ey, near ? dists[ui(0, 6)] : uf(7.f, 500.f), counts[ui(0, 6)]);
        }
        in.hdr[in.lane] = in.h0;  // (the lane's own header is the one it published)
        if (family == 2 && ui(0, 3) == 0) in.hdr[ui(0, 63)] = F4{NAN, in.ey, as_float(5), 0.f};
        int kind = -1;
        const Former want = former_kernel(in), got = from_decision(in, &kind);
        if (kind >= 0 && kind < 5) kinds[kind]++;
        if (!same(want, got)) {
            if (bad < 5)
                std::printf("# %s case %d: state %d/%d reason %d/%d ncp %d/%d own %d/%d set %d/%d src %d/%d move %08x/%08x margin %08x/%08x\n", name,
                            c, want.state, got.state, want.reason, got.reason, want.ncp, got.ncp, want.own, got.own, want.set, got.set,
                            want.src_lane, got.src_lane, bits(want.move), bits(got.move), bits(want.margin), bits(got.margin));
            bad++;
        }
    }
    std::printf("decide %s cases %d bad %d far %d fallback %d afresh %d own %d row %d\n", name, cases, bad, kinds[0], kinds[1], kinds[2],
                kinds[3], kinds[4]);
    return bad;
}

int main() {
    int bad = 0;
    bad += run_family("ordinary_step", 11u, 1500, 0);
    bad += run_family("far_test", 12u, 1500, 1);
    bad += run_family("donors", 13u, 2000, 2);
    bad += run_family("stored_quaternions", 14u, 1500, 3);
    bad += run_family("every_row", 15u, 1000, 4);
    return bad ? 1 : 0;
}
