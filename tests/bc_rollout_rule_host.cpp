// Host program of csrc/bc_rollout_rule.hpp: the closed-loop driver's per-row bookkeeping and summary on scripted sequences,
// with the engine's own order of calls (gd_bc_rollout): start, then per step pre(t) and post(t) while the iteration exists,
// then the summary.  Usage: bc_rollout_rule_host in.bin out.bin
//   in:  int32 N, T;  done [T + 1][N] int32, info [T + 1][N][5] int32, xy [T + 1][N][2] float32, where state 0 is the reset
//        state and state t + 1 what is read after step t (xy: ego columns 3 and 4 of the packed observation of that state)
//   out: dead [N] int32, goal_achieved, off_road, veh_collision [N] f32, goal_step, off_road_step [N] int32, init_goal_dist,
//        goal_dist [N] f32, any_alive [92] int32, summary [8] f32
// Compile without contraction (-ffp-contract=off).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gpudrive_lab_amd/csrc/bc_rollout_rule.hpp"

namespace R = gd::bc_rollout_rule;

template <class V>
static bool read_all(FILE *f, std::vector<V> &v) {
    return v.empty() || fread(v.data(), sizeof(V), v.size(), f) == v.size();
}

template <class V>
static void write_all(FILE *f, const std::vector<V> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(V), v.size(), f) != v.size()) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    int32_t hdr[2];
    if (!f || fread(hdr, 4, 2, f) != 2) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const int N = hdr[0], T = hdr[1];
    if (N < 0 || N > (1 << 20) || T < 1 || T > 91) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const size_t S = static_cast<size_t>(T) + 1;
    std::vector<int32_t> done(S * N), info(S * N * 5);
    std::vector<float> xy(S * N * 2);
    if (!read_all(f, done) || !read_all(f, info) || !read_all(f, xy)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    std::vector<R::Row> rows(N, R::fresh());
    std::vector<int32_t> any_alive(92, 0);
    for (int n = 0; n < N; n++) {  // k_bc_post(-1)
        R::start(rows[n], &info[static_cast<size_t>(n) * 5]);
        any_alive[0] = 1;
    }
    for (int t = 0; t < T; t++) {
        if (!any_alive[t]) continue;  // the iteration does not exist: the kernels return at once
        const size_t s0 = static_cast<size_t>(t) * N, s1 = s0 + N;
        for (int n = 0; n < N; n++) R::pre(rows[n], t, &info[(s0 + n) * 5], xy[(s0 + n) * 2], xy[(s0 + n) * 2 + 1]);
        for (int n = 0; n < N; n++) {
            R::post(rows[n], done[s1 + n], &info[(s1 + n) * 5]);
            if (t + 1 < T && !rows[n].dead) any_alive[t + 1] = 1;
        }
    }
    std::vector<float> partials(R::LANES * 4), summary(R::SUMMARY);
    for (int l = 0; l < R::LANES; l++) R::lane_sums(l, N, [&](int n) { return rows[n]; }, &partials[l * 4]);
    R::finish(partials.data(), N, any_alive.data(), 91, summary.data());

    std::vector<int32_t> dead(N), goal_step(N), off_road_step(N);
    std::vector<float> goal(N), off(N), veh(N), init(N), dist(N);
    for (int n = 0; n < N; n++) {
        dead[n] = rows[n].dead, goal_step[n] = rows[n].goal_step, off_road_step[n] = rows[n].off_road_step;
        goal[n] = rows[n].goal_achieved, off[n] = rows[n].off_road, veh[n] = rows[n].veh_collision;
        init[n] = rows[n].init_goal_dist, dist[n] = rows[n].goal_dist;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    write_all(o, dead), write_all(o, goal), write_all(o, off), write_all(o, veh), write_all(o, goal_step), write_all(o, off_road_step);
    write_all(o, init), write_all(o, dist), write_all(o, any_alive), write_all(o, summary);
    fclose(o);
    return 0;
}
