// Host program of csrc/multi_policy_rule.hpp: the arithmetic the kernels of the multi-policy evaluator run, on files.
//   multi_policy_rule_host starts  in out   in: int32 P, count[P].  out: int32 start[P + 1], then segment_of(q) for every
//                                           position q of a list of n = sum(count) rows, [n + 32 P]
//   multi_policy_rule_host metrics in out   in: int32 W, A, P; int32 owner[W][A] (-1: the slot is no row); float32
//                                           goal_achieved, collided, off_road [W][A]; float32 denominator[W].
//                                           out: float32 [P][7][W] (goal_achieved_count, frac_goal_achieved, collided_count,
//                                           frac_collided, off_road_count, frac_off_road, n_rows), then the summary [P][4]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/multi_policy_rule.hpp"

namespace MP = gd::multi_policy_rule;

static std::vector<char> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    std::vector<char> data;
    char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + k);
    fclose(f);
    return data;
}

template <class T>
static std::vector<T> take(const std::vector<char> &data, size_t &at, size_t n) {
    if (at + n * sizeof(T) > data.size()) exit(3);
    std::vector<T> v(n);
    if (n) memcpy(v.data(), data.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
}

template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(4);
}

int main(int argc, char **argv) {
    if (argc != 4) return 1;
    const std::vector<char> data = slurp(argv[2]);
    size_t at = 0;
    FILE *out = fopen(argv[3], "wb");
    if (!out) return 2;
    if (!strcmp(argv[1], "starts")) {
        const int P = take<int32_t>(data, at, 1)[0];
        if (P < 1 || P > MP::MAX_POLICIES) return 5;
        const std::vector<int32_t> count = take<int32_t>(data, at, P);
        std::vector<int32_t> start(P + 1);
        MP::segment_starts(P, count.data(), start.data());
        int n = 0;
        for (int p = 0; p < P; p++) n += count[p];
        const int limit = MP::list_positions(n, P);
        std::vector<int32_t> seg(limit);
        for (int q = 0; q < limit; q++) seg[q] = MP::segment_of(q, P, start.data(), count.data(), limit);
        put(out, start);
        put(out, seg);
    } else if (!strcmp(argv[1], "metrics")) {
        const std::vector<int32_t> head = take<int32_t>(data, at, 3);
        const int W = head[0], A = head[1], P = head[2];
        if (W < 1 || A < 1 || P < 1 || P > MP::MAX_POLICIES) return 5;
        const size_t S = (size_t)W * A;
        const std::vector<int32_t> owner = take<int32_t>(data, at, S);
        const std::vector<float> goal = take<float>(data, at, S), collided = take<float>(data, at, S), off_road = take<float>(data, at, S);
        const std::vector<float> denominator = take<float>(data, at, W);
        std::vector<float> world((size_t)P * 7 * W), summary((size_t)P * MP::SUMMARY);
        for (int p = 0; p < P; p++) {
            float *o = world.data() + (size_t)p * 7 * W;
            for (int w = 0; w < W; w++) {
                int c[4] = {0, 0, 0, 0};
                for (int a = 0; a < A; a++) {
                    const size_t i = (size_t)w * A + a;
                    if (owner[i] != p) continue;
                    c[0] += goal[i] > 0.f, c[1] += collided[i] > 0.f, c[2] += off_road[i] > 0.f, c[3] += 1;
                }
                const MP::World r = MP::world_counts(c[0], c[1], c[2], c[3], denominator[w]);
                o[0 * W + w] = r.goal_achieved_count, o[1 * W + w] = r.frac_goal_achieved;
                o[2 * W + w] = r.collided_count, o[3 * W + w] = r.frac_collided;
                o[4 * W + w] = r.off_road_count, o[5 * W + w] = r.frac_off_road;
                o[6 * W + w] = r.n_rows;
            }
            std::vector<float> part((size_t)MP::LANES * MP::SUMMARY);
            for (int l = 0; l < MP::LANES; l++)
                MP::lane_sums(l, W, o + 0 * W, o + 2 * W, o + 4 * W, o + 6 * W, part.data() + (size_t)l * MP::SUMMARY);
            MP::finish(part.data(), summary.data() + (size_t)p * MP::SUMMARY);
        }
        put(out, world);
        put(out, summary);
    } else {
        return 1;
    }
    return fclose(out) ? 4 : 0;
}
