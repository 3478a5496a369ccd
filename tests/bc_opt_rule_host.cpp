// Host program of the device BC update's rule (gpudrive_lab_amd/csrc/bc_opt_rule.hpp), built with g++ by
// tests/bc_update_reference.py.  bc_opt_rule_host rows|adamw IN OUT.
//   rows:  IN holds int32 n; then nll [n], actions [n][3], expert [n][3] float32.  OUT receives loss, dx, dy, dyaw and
//          grad_nll [n], float32.
//   adamw: IN holds int32 G, T, steps, step; float32 max_norm, eps, lr, weight_decay; float64 beta1, beta2, pow1, pow2; int32
//          tensor_end [T]; params, exp_avg, exp_avg_sq [G] float32; then `steps` gradients [G] float32.  OUT receives, after
//          every step, params, exp_avg, exp_avg_sq [G] and tensor_norms [T] float32, total and max_grad_norm float32, step and
//          max_grad_tensor int32, pow1, pow2 float64.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/bc_opt_rule.hpp"

namespace R = gd::bc_opt_rule;
namespace P = gd::ppo_rule;

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

static int rows(FILE *in, FILE *out) {
    int32_t n;
    if (!rd(in, &n, 1) || n < 1) return 4;
    std::vector<float> nll(n), act(3 * (size_t)n), ex(3 * (size_t)n), w(n);
    if (!rd(in, nll.data(), nll.size()) || !rd(in, act.data(), act.size()) || !rd(in, ex.data(), ex.size())) return 4;
    float stats[4];
    stats[R::LOSS] = R::mean_of(P::ordered_sum(n, [&](long long i) { return nll[i]; }), n);
    for (int d = 0; d < 3; d++)
        stats[R::DX_LOSS + d] = R::mean_of(P::ordered_sum(n, [&](long long i) { return R::abs_error(act[3 * i + d], ex[3 * i + d]); }), n);
    for (int i = 0; i < n; i++) w[i] = R::grad_nll_of(n);
    wr(out, stats, 4), wr(out, w.data(), w.size());
    return 0;
}

static int adamw(FILE *in, FILE *out) {
    int32_t head[4];
    float hy[4];
    double dd[4];
    if (!rd(in, head, 4) || !rd(in, hy, 4) || !rd(in, dd, 4) || head[0] < 1 || head[1] < 1 || head[2] < 0) return 4;
    const int G = head[0], T = head[1], steps = head[2];
    int32_t step = head[3];
    const float max_norm = hy[0], eps = hy[1], lr = hy[2], weight_decay = hy[3];
    const double beta1 = dd[0], beta2 = dd[1];
    double pw[2] = {dd[2], dd[3]};
    std::vector<int32_t> end(T);
    if (!rd(in, end.data(), T)) return 4;
    for (int t = 0; t < T; t++)
        if (end[t] < (t ? end[t - 1] : 0) || end[t] > G) return 4;
    std::vector<float> p(G), m(G), v(G), g(G), norms(T);
    if (!rd(in, p.data(), G) || !rd(in, m.data(), G) || !rd(in, v.data(), G)) return 4;
    const P::AdamCoefs c = P::adam_coefs(beta1, beta2, eps);
    for (int s = 0; s < steps; s++) {
        if (!rd(in, g.data(), G)) return 4;
        double sum_sq = 0.0;
        for (int t = 0; t < T; t++) {
            const int lo = t ? end[t - 1] : 0;
            const double st = P::ordered_sum(end[t] - lo, [&](long long i) { return R::square(g[lo + i]); });
            norms[t] = R::tensor_norm(st);
            sum_sq += st;
        }
        pw[0] *= beta1, pw[1] *= beta2, step += 1;
        const P::StepScalars sc = P::step_scalars(sum_sq, max_norm, pw[0], pw[1]);
        const R::MaxNorm mx = R::max_norm_of(norms, T, sc.coef);
        const float decay = R::decay_of(lr, weight_decay);
        for (int e = 0; e < G; e++) R::adamw(c, sc, lr, decay, g[e], p[e], m[e], v[e]);
        const int32_t arg = mx.tensor;
        wr(out, p.data(), G), wr(out, m.data(), G), wr(out, v.data(), G), wr(out, norms.data(), T);
        wr(out, &sc.total, 1), wr(out, &mx.value, 1), wr(out, &step, 1), wr(out, &arg, 1), wr(out, pw, 2);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 3;
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 5;
    const int rc = !std::strcmp(argv[1], "rows") ? rows(in, out) : !std::strcmp(argv[1], "adamw") ? adamw(in, out) : 2;
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 5;
}
