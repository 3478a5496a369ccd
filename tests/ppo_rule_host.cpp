// Host program of the device PPO update's rule (gpudrive_lab_amd/csrc/ppo_rule.hpp), built with g++ by
// tests/ppo_update_reference.py.  ppo_rule_host loss|adam IN OUT.
//   loss: IN holds int32 M, norm_adv, clip_vloss; float32 clip_coef, vf_clip_coef, ent_coef, vf_coef; then newlogprob, entropy,
//         newvalue, old_logprob, old_value, adv, ret [M] float32.  OUT receives d_logprob, d_entropy, d_value [M] and the six
//         statistics, float32.
//   adam: IN holds int32 G, steps, step; float32 max_norm, eps, lr; float64 beta1, beta2, pow1, pow2; params, exp_avg,
//         exp_avg_sq [G] float32; then `steps` gradients [G] float32.  OUT receives, after every step, params, exp_avg,
//         exp_avg_sq [G] float32, total float32, step int32, pow1, pow2 float64.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/ppo_rule.hpp"

namespace R = gd::ppo_rule;

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

static int loss(FILE *in, FILE *out) {
    int32_t head[3];
    float hy[4];
    if (!rd(in, head, 3) || !rd(in, hy, 4) || head[0] < 1) return 4;
    const int m = head[0];
    const R::Hyper h{hy[0], hy[1], hy[2], hy[3], head[1] != 0, head[2] != 0};
    std::vector<float> x[7];
    for (auto &v : x) {
        v.resize(m);
        if (!rd(in, v.data(), m)) return 4;
    }
    const float *nlp = x[0].data(), *ent = x[1].data(), *nv = x[2].data(), *olp = x[3].data(), *ov = x[4].data(), *adv = x[5].data(),
                *ret = x[6].data();
    R::Norm nm{0.f, 1.f};
    if (h.norm_adv) {
        if (m < 2) return 4;
        const float mean = R::mean_of(R::ordered_sum(m, [&](long long i) { return adv[i]; }), m);
        nm = R::norm_of(mean, R::ordered_sum(m, [&](long long i) { return R::centred_square(adv[i], mean); }), m);
    }
    const float inv_m = 1.f / (float)m;
    std::vector<R::Row> rows(m);
    for (int i = 0; i < m; i++) rows[i] = R::row(h, nm, inv_m, nlp[i], nv[i], olp[i], ov[i], adv[i], ret[i]);
    std::vector<float> d[3];
    for (auto &v : d) v.resize(m);
    for (int i = 0; i < m; i++) d[0][i] = rows[i].d_logprob, d[1][i] = rows[i].d_entropy, d[2][i] = rows[i].d_value;
    float stats[6];
    stats[R::POLICY_LOSS] = R::mean_of(R::ordered_sum(m, [&](long long i) { return rows[i].pg; }), m);
    stats[R::VALUE_LOSS] = 0.5f * R::mean_of(R::ordered_sum(m, [&](long long i) { return rows[i].vl; }), m);
    stats[R::ENTROPY] = R::mean_of(R::ordered_sum(m, [&](long long i) { return ent[i]; }), m);
    stats[R::OLD_APPROX_KL] = R::mean_of(R::ordered_sum(m, [&](long long i) { return rows[i].neg_logratio; }), m);
    stats[R::APPROX_KL] = R::mean_of(R::ordered_sum(m, [&](long long i) { return rows[i].kl; }), m);
    stats[R::CLIPFRAC] = R::mean_of(R::ordered_sum(m, [&](long long i) { return rows[i].clipped; }), m);
    for (auto &v : d) wr(out, v.data(), m);
    wr(out, stats, 6);
    return 0;
}

static int adam(FILE *in, FILE *out) {
    int32_t head[3];
    float hy[3];
    double dd[4];
    if (!rd(in, head, 3) || !rd(in, hy, 3) || !rd(in, dd, 4) || head[0] < 1 || head[1] < 0) return 4;
    const int G = head[0], steps = head[1];
    int32_t step = head[2];
    const float max_norm = hy[0], eps = hy[1], lr = hy[2];
    const double beta1 = dd[0], beta2 = dd[1];
    double pw[2] = {dd[2], dd[3]};
    std::vector<float> p(G), m(G), v(G), g(G);
    if (!rd(in, p.data(), G) || !rd(in, m.data(), G) || !rd(in, v.data(), G)) return 4;
    const R::AdamCoefs c = R::adam_coefs(beta1, beta2, eps);
    for (int s = 0; s < steps; s++) {
        if (!rd(in, g.data(), G)) return 4;
        const double sum_sq = R::ordered_sum(G, [&](long long e) { return g[e] * g[e]; });
        pw[0] *= beta1, pw[1] *= beta2, step += 1;
        const R::StepScalars sc = R::step_scalars(sum_sq, max_norm, pw[0], pw[1]);
        for (int e = 0; e < G; e++) R::adam(c, sc, lr, g[e], p[e], m[e], v[e]);
        wr(out, p.data(), G), wr(out, m.data(), G), wr(out, v.data(), G);
        wr(out, &sc.total, 1), wr(out, &step, 1), wr(out, pw, 2);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 3;
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 5;
    const int rc = !std::strcmp(argv[1], "loss") ? loss(in, out) : !std::strcmp(argv[1], "adam") ? adam(in, out) : 2;
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 5;
}
