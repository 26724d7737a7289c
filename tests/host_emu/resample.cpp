// driver of the host build of csrc/resample.hip (kernels.h beside it): small shapes against straightforward f64 loops of tasks/gqa_resampling.py:184-203
// and of the closed-form weight gradient with torch.optim.SGD's momentum update.  Every operand sits in an allocation of exactly its size (a sanitizer
// build sees any access past it), outputs carry guard words, and each case runs twice - operands 16-byte aligned with pitches that allow 16-byte
// accesses, and shifted by one float with odd pitches - and must give the same bits.
#include "rgqa_amd/csrc/resample.cpp"
#include <random>
static std::mt19937 rng(1);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
struct Out { std::vector<float> weights, loss, dl, rl, theta, buf, g; double stats[2]; };
static double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }

// layout 0: aligned, pitches multiples of 4; layout 1: every float operand one float off, odd pitches
static int run(int layout, int N, int n_pos, int Bn, int NA, int NAp, const std::vector<float>& theta, const std::vector<int64_t>& wid, const std::vector<float>& z,
               const std::vector<float>& t, float gs, float lr, float mom, const std::vector<float>& buf0, Out& o) {
    const int B = n_pos + Bn, off = layout;
    const int ld = layout ? NA + 3 + (NA % 2 == 0) : (NA + 3) / 4 * 4 + 4, ldt = NA + 1, ldd = layout ? NAp + 1 + (NAp % 2 == 0) : (NAp + 3) / 4 * 4;
    std::vector<float> zb(off + (size_t)ld * (B - 1) + NA), tb(off + (size_t)ldt * (B - 1) + NA + 1), db(off + (size_t)ldd * B, 7.f);
    for (int b = 0; b < B; ++b) { memcpy(&zb[off + (size_t)b * ld], &z[(size_t)b * NA], 4 * NA); memcpy(&tb[off + (size_t)b * ldt], &t[(size_t)b * (NA + 1)], 4 * (NA + 1)); }
    const size_t ns = k_resample_scratch_floats(N, B);
    std::vector<float> scratch(off + ns + 8, 5.f);
    std::vector<float> th(off + N), bf(off + N), gr(off + N + 4, 3.f), wts(off + Bn + 4, 9.f), rl(off + Bn + 4, 9.f), loss(off + 3 + 2, 9.f);
    memcpy(&th[off], theta.data(), 4 * (size_t)N); memcpy(&bf[off], buf0.data(), 4 * (size_t)N);
    std::vector<int64_t> wd(wid);                         // exactly Bn entries
    double stats[4] = {0, 0, 11.0, 11.0};
    int bad = 0;
    if (k_resample_weights(&th[off], N, wd.data(), Bn, stats, &wts[off], &scratch[off], nullptr)) return 1000;
    if (k_resample_loss(&zb[off], ld, &tb[off], ldt, B, n_pos, NA, NAp, &wts[off], gs, &loss[off], &db[off], ldd, &rl[off], &scratch[off], nullptr)) return 1000;
    if (k_resample_step(&th[off], &bf[off], N, wd.data(), &rl[off], Bn, stats, lr, mom, &gr[off], &scratch[off], nullptr)) return 1000;
    for (size_t i = off + ns; i < off + ns + 8; ++i) if (scratch[i] != 5.f) ++bad;
    for (int i = 0; i < 4; ++i) if (wts[off + Bn + i] != 9.f || rl[off + Bn + i] != 9.f || gr[off + N + i] != 3.f) ++bad;
    if (loss[off + 3] != 9.f || loss[off + 4] != 9.f || stats[2] != 11.0 || stats[3] != 11.0) ++bad;
    for (int i = 0; i < off; ++i) if (db[i] != 7.f || wts[i] != 9.f || rl[i] != 9.f || gr[i] != 3.f || loss[i] != 9.f || scratch[i] != 5.f) ++bad;
    o.dl.assign((size_t)B * NAp, 0.f);
    for (int b = 0; b < B; ++b) {
        for (int n = 0; n < NAp; ++n) o.dl[(size_t)b * NAp + n] = db[off + (size_t)b * ldd + n];
        for (int n = NAp; n < ldd && (size_t)off + (size_t)b * ldd + n < db.size(); ++n) if (db[off + (size_t)b * ldd + n] != 7.f) ++bad;
    }
    o.weights.assign(wts.begin() + off, wts.begin() + off + Bn); o.rl.assign(rl.begin() + off, rl.begin() + off + Bn); o.loss.assign(loss.begin() + off, loss.begin() + off + 3);
    o.theta.assign(th.begin() + off, th.end()); o.buf.assign(bf.begin() + off, bf.end()); o.g.assign(gr.begin() + off, gr.begin() + off + N);
    o.stats[0] = stats[0]; o.stats[1] = stats[1];
    if (bad) printf("guard words overwritten (%d)\n", bad);
    return bad;
}

static bool same(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), 4 * a.size()); }

// stray: replace two indices by ones outside [0, N) - they must be skipped (weight 0, no share in the gradient) and nothing outside the arrays touched
static int check(int N, int n_pos, int Bn, int NA, int NAp, bool stray = false, bool once = false) {
    const int B = n_pos + Bn;
    std::vector<float> theta(N), buf0(N), z((size_t)B * NA), t((size_t)B * (NA + 1), 0.f);
    for (auto& v : theta) v = 2.f * rnd();
    for (auto& v : buf0) v = 0.01f * rnd();
    if (N >= 3) { theta[N / 2] = 25.f; theta[N - 1] = -12.f; }
    std::vector<int64_t> wid(Bn);
    for (int b = 0; b < Bn; ++b) wid[b] = rng() % N;
    if (Bn >= 3) { wid[0] = N / 2; wid[Bn - 1] = N - 1; wid[1] = 0; }
    if (Bn >= 7) { wid[2] = wid[4] = wid[6] = (N / 3) % N; }            // one index three times
    if (stray) { wid[3] = -1; wid[5] = N; }
    for (auto& v : z) v = 3.f * rnd() - 6.f;
    for (int b = 0; b < B; ++b) {
        if (b < n_pos) { t[(size_t)b * (NA + 1) + (b * 7) % NA] = 0.9f; t[(size_t)b * (NA + 1) + (b * 7 + 3) % NA] = 0.3f; }
        else t[(size_t)b * (NA + 1) + NA] = 1.f;
    }
    const float lr = 0.5f, mom = 0.9f;
    // ---- f64 reference
    std::vector<double> w(N), wt(Bn), r(B), s(N, 0.0);
    double m1 = 0, mh = 0;
    for (int j = 0; j < N; ++j) { w[j] = softplus_d(theta[j]); m1 += w[j]; mh += sqrt(w[j]); }
    m1 /= N; mh /= N;
    auto ok = [&](int64_t j) { return j >= 0 && j < N; };
    for (int b = 0; b < Bn; ++b) wt[b] = ok(wid[b]) ? mh / m1 * sqrt(w[wid[b]]) : 0.0;
    double lp = 0, ln = 0, S = 0;
    for (int b = 0; b < B; ++b) {
        double a = 0;
        for (int n = 0; n < NA; ++n) { const double x = z[(size_t)b * NA + n], y = t[(size_t)b * (NA + 1) + n]; a += std::max(x, 0.0) - x * y + log1p(exp(-fabs(x))); }
        r[b] = a;
        if (b < n_pos) lp += a; else { ln += wt[b - n_pos] * a; if (ok(wid[b - n_pos])) { S += a * sqrt(w[wid[b - n_pos]]); s[wid[b - n_pos]] += a; } }
    }
    lp /= n_pos; ln /= Bn;
    Out o0, o1, o2;
    int bad = 0;
    if (once) { bad = run(1, N, n_pos, Bn, NA, NAp, theta, wid, z, t, 1.0f, lr, mom, buf0, o0); o1 = o0; o2 = o0; for (auto& v : o2.dl) v *= 0.5f; }
    else bad = run(0, N, n_pos, Bn, NA, NAp, theta, wid, z, t, 1.0f, lr, mom, buf0, o0) + run(1, N, n_pos, Bn, NA, NAp, theta, wid, z, t, 1.0f, lr, mom, buf0, o1)
               + run(1, N, n_pos, Bn, NA, NAp, theta, wid, z, t, 0.5f, lr, mom, buf0, o2);
    if (!same(o0.weights, o1.weights) || !same(o0.loss, o1.loss) || !same(o0.dl, o1.dl) || !same(o0.rl, o1.rl) || !same(o0.theta, o1.theta) || !same(o0.buf, o1.buf) || !same(o0.g, o1.g)
        || o0.stats[0] != o1.stats[0] || o0.stats[1] != o1.stats[1]) { printf("the two layouts differ\n"); ++bad; }
    auto close = [](double g, double ref, double tol) { return std::fabs(g - ref) <= tol * std::fabs(ref) + 1e-30; };
    if (!close(o0.stats[0], m1, 1e-12) || !close(o0.stats[1], mh, 1e-12)) { printf("stats got %.17g %.17g ref %.17g %.17g\n", o0.stats[0], o0.stats[1], m1, mh); ++bad; }
    if (!close(o0.loss[0], lp + ln, 1e-6) || !close(o0.loss[1], lp, 1e-6) || !close(o0.loss[2], ln, 1e-6)) { printf("loss got %.9g %.9g %.9g ref %.9g %.9g %.9g\n", o0.loss[0], o0.loss[1], o0.loss[2], lp + ln, lp, ln); ++bad; }
    double wmax = 0; for (double v : wt) wmax = std::max(wmax, v);
    for (int b = 0; b < Bn; ++b) {
        if (std::fabs(o0.weights[b] - wt[b]) > 1e-6 * wmax) { printf("weights[%d] got %.9g ref %.9g\n", b, o0.weights[b], wt[b]); ++bad; }
        if (!ok(wid[b]) && o0.weights[b] != 0.f) { printf("a stray index has a weight\n"); ++bad; }
        if (!close(o0.rl[b], r[n_pos + b], 1e-6)) { printf("row_loss[%d] got %.9g ref %.9g\n", b, o0.rl[b], r[n_pos + b]); ++bad; }
    }
    double dmax = 0;
    std::vector<double> dref((size_t)B * NAp, 0.0);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < NA; ++n) {
            const double x = z[(size_t)b * NA + n], y = t[(size_t)b * (NA + 1) + n], cb = b < n_pos ? 1.0 / n_pos : wt[b - n_pos] / Bn;
            dref[(size_t)b * NAp + n] = (1.0 / (1.0 + exp(-x)) - y) * cb;
            dmax = std::max(dmax, std::fabs(dref[(size_t)b * NAp + n]));
        }
    for (size_t i = 0; i < dref.size(); ++i) {
        if (std::fabs(o0.dl[i] - dref[i]) > 2e-6 * dmax) { if (bad < 5) printf("dlogits[%zu] got %.9g ref %.9g (max %.3g)\n", i, o0.dl[i], dref[i], dmax); ++bad; }
        if ((int)(i % NAp) >= NA && (o0.dl[i] != 0.f || std::signbit(o0.dl[i]))) { printf("padding not +0\n"); ++bad; }
        if (o2.dl[i] != 0.5f * o0.dl[i]) { if (bad < 5) printf("grad_scale 0.5 does not halve dlogits[%zu]\n", i); ++bad; }
    }
    // the weight step (from the f64 row sums: the kernels' f32 row_loss differs from them by rounding only)
    std::vector<double> g(N), bn(N), tn(N);
    double gmax = 0, bmax = 0;
    for (int j = 0; j < N; ++j) {
        const double sq = sqrt(w[j]), dw = -(S / (2.0 * N * m1 * sq) - mh * S / (N * m1 * m1) + mh / (2.0 * m1) * s[j] / sq) / Bn;
        g[j] = dw * (theta[j] > 20.f ? 1.0 : 1.0 / (1.0 + exp(-(double)theta[j])));
        bn[j] = (double)mom * buf0[j] + g[j]; tn[j] = theta[j] - (double)lr * bn[j];
        gmax = std::max(gmax, std::fabs(g[j])); bmax = std::max(bmax, std::fabs(bn[j]));
    }
    int moved = 0;
    for (int j = 0; j < N; ++j) {
        if (std::fabs(o0.g[j] - g[j]) > 2e-6 * gmax) { if (bad < 5) printf("g[%d] got %.9g ref %.9g (max %.3g)\n", j, o0.g[j], g[j], gmax); ++bad; }
        if (std::fabs(o0.buf[j] - bn[j]) > 2e-6 * bmax) { if (bad < 5) printf("buf[%d] got %.9g ref %.9g\n", j, o0.buf[j], bn[j]); ++bad; }
        if (std::fabs(o0.theta[j] - tn[j]) > 2e-6 * lr * bmax + 1.2e-7 * std::fabs(tn[j])) { if (bad < 5) printf("theta[%d] got %.9g ref %.9g\n", j, o0.theta[j], tn[j]); ++bad; }
        moved += o0.g[j] != 0.f;
    }
    if (N > 1 && moved != N) { printf("the gradient is dense: %d of %d entries non-zero\n", moved, N); ++bad; }
    printf("resample N=%d n_pos=%d Bn=%d NA=%d NAp=%d stray=%d: %d bad\n", N, n_pos, Bn, NA, NAp, (int)stray, bad);
    return bad;
}
int main(int argc, char** argv) {
    // a workgroup costs 256 host threads: the default set keeps to ~120 of them (seconds); "full" adds the larger shapes
    const bool full = argc > 1 && !strcmp(argv[1], "full");
    int bad = 0;
    bad += check(2, 2, 3, 67, 128);
    bad += check(37, 2, 7, 67, 128);
    bad += check(4099, 1, 7, 1842, 1856, false, true);        // more than one quad sweep per row, five chunks of theta (the last one partial)
    bad += check(37, 3, 9, 67, 67, true, true);               // stray indices; NAp = NA, not a multiple of 4
    if (full) {
        bad += check(4099, 5, 7, 300, 320);
        bad += check(3, 1, 1, 67, 128);
        bad += check(37, 150, 150, 67, 67, false, true);      // more rows than the 256 threads of the fold
        bad += check(37, 2, 300, 5, 8, false, true);          // Bn > 256: two sweeps of the owner pass
    }
    float x[8] = {0}; double st[2]; int64_t wd[2] = {0, 0};
    if (k_resample_loss(x, 4, x, 4, 2, 0, 4, 4, x, 1.f, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0) { printf("n_pos = 0 accepted\n"); ++bad; }
    if (k_resample_loss(x, 4, x, 4, 2, 2, 4, 4, x, 1.f, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0) { printf("n_pos = B accepted\n"); ++bad; }
    if (k_resample_loss(x, 4, x, 4, 2, 1, 4, 4, x, 1.f, x, nullptr, 0, nullptr, nullptr, nullptr) == 0) { printf("loss without scratch accepted\n"); ++bad; }
    if (k_resample_loss(x, 4, x, 4, 2, 1, 4, 8, x, 1.f, nullptr, x, 4, nullptr, nullptr, nullptr) == 0) { printf("ldd < NAp accepted\n"); ++bad; }
    if (k_resample_weights(x, 0, wd, 1, st, x, x, nullptr) == 0) { printf("N = 0 accepted\n"); ++bad; }
    if (k_resample_step(x, x, 4, wd, x, 0, st, 1.f, 0.9f, nullptr, x, nullptr) == 0) { printf("Bn = 0 accepted\n"); ++bad; }
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
