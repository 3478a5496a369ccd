// The host program of gpudrive_lab_amd/csrc/lp_rule.hpp: the linear probe's rule on plain arrays, for tests/probe_cases.py.
// Built with g++ -ffp-contract=off.  usage: lp_rule_host in.bin out.bin; in.bin starts with an int32 mode:
//   0 rows    [mode, n, exp] int32; logits [n][64] f32; labels [n] int64; mask [n] u8
//             -> per row pred int32, loss_row f32, g [64] f32; then int32 M, correct, bad, ood_correct, ood_rows; the six
//                per-class counters [6][64] int32; loss, accuracy, f1 f32; the loss sum and the OOD loss sum f64
//                (the batch as ONE partial: rows in ascending order)
//   1 reduce  [mode, P, K] int32; part_f [P][64 K + 64] f32; part_d [P][2] f64; part_i [P][392] int32
//             -> M int32; grad [64 K + 64] f32 (zeros when M == 0); stats [8] f32 (zeros when M == 0)
//   2 adamw   [mode, K, steps] int32; lr, eps, weight_decay f32; beta1, beta2 f64; weight, exp_avg, exp_avg_sq [64 K + 64] f32;
//             step int32; beta_pow [2] f64; then per step: M int32, grad [64 K + 64] f32
//             -> weight, exp_avg, exp_avg_sq; step int32; beta_pow [2] f64
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/lp_rule.hpp"

namespace R = gd::lp_rule;
namespace P = gd::ppo_rule;

struct In {
    std::vector<unsigned char> buf;
    size_t at = 0;
    template <class T>
    std::vector<T> vec(size_t n) {
        if (at + n * sizeof(T) > buf.size()) {
            fprintf(stderr, "lp_rule_host: input too short\n");
            exit(2);
        }
        std::vector<T> v(n);
        if (n) memcpy(v.data(), buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

template <class T>
static void put(FILE *f, const T *p, size_t n) {
    fwrite(p, sizeof(T), n, f);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    In in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        in.buf.resize(ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(in.buf.data(), 1, in.buf.size(), f) != in.buf.size()) return 2;
        fclose(f);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const std::vector<int32_t> hd = in.vec<int32_t>(3);
    const int mode = hd[0];
    if (mode == 0) {
        const int n = hd[1], exp = hd[2];
        const std::vector<float> z = in.vec<float>((size_t)n * 64);
        const std::vector<int64_t> labels = in.vec<int64_t>(n);
        const std::vector<unsigned char> mask = in.vec<unsigned char>(n);
        int32_t head[5] = {0, 0, 0, 0, 0}, cnt[R::N_COUNTERS][R::CLASSES];
        memset(cnt, 0, sizeof cnt);
        double loss = 0.0, ood_loss = 0.0;
        for (int i = 0; i < n; i++) {
            const float *zr = z.data() + (size_t)i * 64;
            const R::Row row = R::row([&](int c) { return zr[c]; });
            const bool ok = R::label_ok(labels[i]), sel = R::selected(exp, mask[i]), use = ok && sel;
            const int lab = ok ? (int)labels[i] : 0;
            const float lr = ok ? R::loss_row(row, zr[lab]) : 0.f;
            float g[64];
            for (int c = 0; c < 64; c++) g[c] = use ? R::grad(row, zr[c], c == lab) : 0.f;
            const int32_t pred = row.pred;
            put(out, &pred, 1), put(out, &lr, 1), put(out, g, 64);
            head[2] += sel && !ok;
            if (!use) continue;
            loss += (double)lr;
            head[0]++, head[1] += pred == lab;
            cnt[R::C_TP][lab] += pred == lab, cnt[R::C_PRED][pred]++, cnt[R::C_LABEL][lab]++;
            if (R::ood(exp, lab)) {
                ood_loss += (double)lr;
                head[4]++, head[3] += pred == lab;
                cnt[R::C_OOD_TP][lab] += pred == lab, cnt[R::C_OOD_PRED][pred]++, cnt[R::C_OOD_LABEL][lab]++;
            }
        }
        float st[3] = {0.f, 0.f, 0.f};
        if (head[0] > 0) {
            st[0] = R::loss_of(loss, head[0]), st[1] = R::accuracy_of(head[1], head[0]);
            st[2] = R::macro_f1([&](int c) { return cnt[R::C_TP][c]; }, [&](int c) { return cnt[R::C_PRED][c]; },
                                [&](int c) { return cnt[R::C_LABEL][c]; });
        }
        put(out, head, 5), put(out, &cnt[0][0], R::N_COUNTERS * R::CLASSES), put(out, st, 3);
        const double d[2] = {loss, ood_loss};
        put(out, d, 2);
    } else if (mode == 1) {
        const int Pn = hd[1], K = hd[2], GF = 64 * K + 64;
        const std::vector<float> pf = in.vec<float>((size_t)Pn * GF);
        const std::vector<double> pd = in.vec<double>((size_t)Pn * 2);
        const std::vector<int32_t> pi = in.vec<int32_t>((size_t)Pn * R::PART_INTS);
        int32_t M = 0, correct = 0, bad = 0, ood_correct = 0, ood_rows = 0;
        double loss = 0.0, ood_loss = 0.0;
        std::vector<int32_t> cnt(R::N_COUNTERS * R::CLASSES, 0);
        for (int w = 0; w < Pn; w++) {
            const int32_t *q = pi.data() + (size_t)w * R::PART_INTS;
            M += q[R::N_ROWS], correct += q[R::N_CORRECT], bad += q[R::N_BAD], ood_correct += q[R::N_OOD_CORRECT], ood_rows += q[R::N_OOD_ROWS];
            loss += pd[(size_t)w * 2], ood_loss += pd[(size_t)w * 2 + 1];
            for (int i = 0; i < R::N_COUNTERS * R::CLASSES; i++) cnt[i] += q[R::N_HEAD + i];
        }
        std::vector<float> grad(GF, 0.f);
        float st[R::N_STATS] = {0};
        if (M > 0) {
            for (int e = 0; e < GF; e++) {
                float s = pf[e];
                for (int w = 1; w < Pn; w++) s = s + pf[(size_t)w * GF + e];
                grad[e] = R::scaled(s, M);
            }
            st[R::S_LOSS] = R::loss_of(loss, M), st[R::S_ACCURACY] = R::accuracy_of(correct, M);
            st[R::S_F1] = R::macro_f1([&](int c) { return cnt[R::C_TP * 64 + c]; }, [&](int c) { return cnt[R::C_PRED * 64 + c]; },
                                      [&](int c) { return cnt[R::C_LABEL * 64 + c]; });
            st[R::S_OOD_LOSS_SUM] = (float)ood_loss, st[R::S_OOD_CORRECT] = (float)ood_correct, st[R::S_OOD_ROWS] = (float)ood_rows;
            st[R::S_ROWS] = (float)M, st[R::S_BAD] = (float)bad;
        }
        put(out, &M, 1), put(out, grad.data(), GF), put(out, st, R::N_STATS);
    } else if (mode == 2) {
        const int K = hd[1], steps = hd[2], GF = 64 * K + 64;
        const std::vector<float> hp = in.vec<float>(3);
        const float lr = hp[0], eps = hp[1], wd = hp[2];
        const std::vector<double> beta = in.vec<double>(2);
        std::vector<float> w = in.vec<float>(GF), m = in.vec<float>(GF), v = in.vec<float>(GF);
        int32_t step = in.vec<int32_t>(1)[0];
        std::vector<double> pw = in.vec<double>(2);
        const P::AdamCoefs c = P::adam_coefs(beta[0], beta[1], eps);
        for (int s = 0; s < steps; s++) {
            const int32_t M = in.vec<int32_t>(1)[0];
            const std::vector<float> g = in.vec<float>(GF);
            if (M <= 0) continue;  // the reference's `continue`
            pw[0] *= beta[0], pw[1] *= beta[1], step++;
            const P::StepScalars sc = R::step_scalars(pw[0], pw[1]);
            const float decay = R::O::decay_of(lr, wd);
            for (int e = 0; e < GF; e++) R::O::adamw(c, sc, lr, decay, g[e], w[e], m[e], v[e]);
        }
        put(out, w.data(), GF), put(out, m.data(), GF), put(out, v.data(), GF), put(out, &step, 1), put(out, pw.data(), 2);
    } else {
        return 2;
    }
    fclose(out);
    return 0;
}
