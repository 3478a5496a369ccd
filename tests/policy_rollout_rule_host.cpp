// Host program of csrc/policy_rollout_rule.hpp: the closed-loop PPO evaluator's bookkeeping on scripted sequences, with the
// engine's own order of calls (gd_policy_rollout): per step, while the iteration exists, the row step of every mask slot, the
// world test, episode_lengths and any_active[t + 1]; then the per-world counts and the summary.
// Usage: policy_rollout_rule_host in.bin out.bin
//   in:  int32 W, A, T;  mask [W][A] int32, done [T][W][A] int32, info [T][W][A][5] int32, entry t what is read after step t
//   out: live [W][A] int32, goal_achieved, collided, off_road [W][A] f32 (slots outside the mask: 0), world_active [W] int32,
//        episode_lengths [W] f32, the nine per-world results [W] f32 each in the header's order, any_active [92] int32,
//        summary [8] f32
// Compile without contraction (-ffp-contract=off).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gpudrive_lab_amd/csrc/policy_rollout_rule.hpp"

namespace R = gd::policy_rollout_rule;

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
    int32_t hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const int W = hdr[0], A = hdr[1], T = hdr[2];
    if (W < 1 || W > 4096 || A < 1 || A > 128 || T < 1 || T > 91) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const size_t S = static_cast<size_t>(W) * A;
    std::vector<int32_t> mask(S), done(S * T), info(S * T * 5);
    if (!read_all(f, mask) || !read_all(f, done) || !read_all(f, info)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(f);

    std::vector<R::Row> rows(S, R::Row{0, 0.f, 0.f, 0.f});
    for (size_t i = 0; i < S; i++)
        if (mask[i]) rows[i] = R::fresh();
    std::vector<int32_t> world_active(W, 1), any_active(92, 0);
    std::vector<float> episode_lengths(W, 0.f);
    any_active[0] = 1;
    for (int t = 0; t < T; t++) {
        if (!any_active[t]) continue;  // the iteration does not exist: the kernels return at once
        for (int w = 0; w < W; w++) {  // k_pr_book: one workgroup per world
            int n_done = 0, n_mask = 0;
            for (int a = 0; a < A; a++) {
                const size_t slot = static_cast<size_t>(w) * A + a, at = static_cast<size_t>(t) * S + slot;
                if (!mask[slot]) continue;
                R::row_step(rows[slot], done[at], &info[at * 5]);
                n_mask++;
                n_done += done[at] != 0;
            }
            if (!world_active[w]) continue;
            if (R::world_done(n_done, n_mask)) {
                episode_lengths[w] = static_cast<float>(t);
                world_active[w] = 0;
            } else {
                any_active[t + 1] = 1;
            }
        }
    }
    std::vector<std::vector<float>> res(9, std::vector<float>(W));
    for (int w = 0; w < W; w++) {  // k_pr_world
        int c[5] = {0, 0, 0, 0, 0};
        for (int a = 0; a < A; a++) {
            const size_t slot = static_cast<size_t>(w) * A + a;
            if (!mask[slot]) continue;
            const int fl = R::row_flags(rows[slot]);
            c[0] += (fl & R::F_GOAL) != 0, c[1] += (fl & R::F_COLLIDED) != 0, c[2] += (fl & R::F_OFF_ROAD) != 0;
            c[3] += (fl & R::F_OTHER) != 0, c[4]++;
        }
        const R::World o = R::world_counts(c[0], c[1], c[2], c[3], c[4]);
        res[0][w] = o.goal_achieved_count, res[1][w] = o.frac_goal_achieved, res[2][w] = o.collided_count;
        res[3][w] = o.frac_collided, res[4][w] = o.off_road_count, res[5][w] = o.frac_off_road, res[6][w] = o.other_count;
        res[7][w] = o.frac_other, res[8][w] = o.controlled;
    }
    std::vector<float> partials(R::LANES * R::PARTIALS), summary(R::SUMMARY);
    for (int l = 0; l < R::LANES; l++)  // k_pr_summary
        R::lane_sums(l, W, res[0].data(), res[2].data(), res[4].data(), res[6].data(), res[8].data(), episode_lengths.data(),
                     &partials[static_cast<size_t>(l) * R::PARTIALS]);
    R::finish(partials.data(), W, any_active.data(), T, summary.data());

    std::vector<int32_t> live(S);
    std::vector<float> goal(S), coll(S), off(S);
    for (size_t i = 0; i < S; i++)
        live[i] = rows[i].live, goal[i] = rows[i].goal_achieved, coll[i] = rows[i].collided, off[i] = rows[i].off_road;
    FILE *o = fopen(argv[2], "wb");
    if (!o) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    write_all(o, live), write_all(o, goal), write_all(o, coll), write_all(o, off), write_all(o, world_active);
    write_all(o, episode_lengths);
    for (const auto &v : res) write_all(o, v);
    write_all(o, any_active), write_all(o, summary);
    fclose(o);
    return 0;
}
