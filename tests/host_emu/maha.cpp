// driver of the host build of csrc/maha.hip (kernels.h beside it): small shapes against straightforward f64 loops
#include "rgqa_amd/csrc/maha.cpp"
#include <random>
static std::mt19937 rng(1);
static float rnd() { return std::normal_distribution<float>(0, 1)(rng); }
int check_score(int B, int H, int R, int NC, bool nanrow) {
    std::vector<float> x(B * (H + 3)), W(H * R), nu(NC * R), y(B * R), sc(B), all(B * (NC + 5), 7.f);
    std::vector<int64_t> lab(B);
    for (auto& v : x) v = rnd(); for (auto& v : W) v = rnd(); for (auto& v : nu) v = rnd();
    for (int r = 0; r < R; ++r) { nu[3 * R + r] = nu[1 * R + r]; }        // duplicated class
    for (int r = 0; r < R; ++r) nu[2 * R + r] = 1e20f;                     // a class whose squared distance overflows f32: -inf, never the winner
    if (nanrow) x[2 * (H + 3) + 1] = NAN;
    size_t sb; rgqa_maha_scratch_bytes(B, NC, &sb);
    std::vector<char> scratch(sb + 64, 0x5a);
    int rc = rgqa_maha_score_rows(x.data(), H + 3, W.data(), nu.data(), B, H, R, NC, y.data(), sc.data(), lab.data(), all.data(), NC + 5, scratch.data(), sb, nullptr);
    if (rc) return 100;
    for (size_t i = sb; i < sb + 64; ++i) if (scratch[i] != 0x5a) { printf("scratch overrun\n"); return 101; }
    int bad = 0;
    for (int b = 0; b < B; ++b) {
        double best = -1e300; int bi = -1; bool isn = false;
        for (int c = 0; c < NC; ++c) {
            double s = 0;
            for (int r = 0; r < R; ++r) { double yy = 0; for (int k = 0; k < H; ++k) yy += (double)x[b * (H + 3) + k] * W[k * R + r]; double d = yy - nu[c * R + r]; s += d * d; }
            s *= -0.5;
            float g = all[b * (NC + 5) + c];
            if (std::isnan(s)) { isn = true; if (!std::isnan(g)) ++bad; continue; }
            if (std::isinf((float)s)) { if (g != (float)s) { printf("overflow class b=%d c=%d got %g\n", b, c, g); ++bad; } continue; }
            if (std::fabs(g - s) > 1e-4 * std::fabs(s) + 1e-4) { if (bad < 5) printf("score mismatch b=%d c=%d got %g ref %g\n", b, c, g, s); ++bad; }
            if (g > best) { best = g; bi = c; }     // first maximum of the device's own values
        }
        for (int c = NC; c < NC + 5; ++c) if (all[b * (NC + 5) + c] != 7.f) { printf("wrote past NC\n"); ++bad; }
        if (isn) { if (!std::isnan(sc[b]) || lab[b] != 0) { printf("nan row b=%d: score %g label %ld\n", b, sc[b], (long)lab[b]); ++bad; } continue; }
        if (lab[b] != bi || sc[b] != (float)best) { printf("argmax mismatch b=%d got %ld (%g) ref %d (%g)\n", b, (long)lab[b], sc[b], bi, best); ++bad; }
    }
    printf("score B=%d H=%d R=%d NC=%d: %d bad\n", B, H, R, NC, bad);
    return bad;
}
int check_dpooled(int B, int H, int R, int NC) {
    std::vector<float> x(B * (H + 2)), W(H * R), mean(NC * H), d(B * R), g(B * (H + 1), 7.f);
    std::vector<int64_t> lab(B);
    for (auto& v : x) v = rnd(); for (auto& v : W) v = rnd(); for (auto& v : mean) v = rnd();
    for (int b = 0; b < B; ++b) lab[b] = (b * 7) % NC;
    lab[1] = NC;   // invalid
    if (rgqa_maha_dpooled(x.data(), H + 2, mean.data(), lab.data(), W.data(), 0.25f, B, H, R, NC, d.data(), g.data(), H + 1, nullptr)) return 100;
    int bad = 0;
    for (int b = 0; b < B; ++b) {
        for (int h = 0; h < H; ++h) {
            double s = 0;
            if (lab[b] < NC) for (int r = 0; r < R; ++r) { double dd = 0; for (int k = 0; k < H; ++k) dd += ((double)x[b * (H + 2) + k] - mean[lab[b] * H + k]) * W[k * R + r]; s += dd * W[h * R + r]; }
            s *= 0.25;
            float got = g[b * (H + 1) + h];
            if (std::fabs(got - s) > 1e-3 * (std::fabs(s) + 1)) { if (bad < 5) printf("dpooled mismatch b=%d h=%d got %g ref %g\n", b, h, got, s); ++bad; }
        }
        if (g[b * (H + 1) + H] != 7.f) { printf("dpooled wrote past H\n"); ++bad; }
    }
    printf("dpooled B=%d H=%d R=%d NC=%d: %d bad\n", B, H, R, NC, bad);
    return bad;
}
int check_acc(int B, int H, int NC) {
    std::vector<float> x(B * (H + 1)), t(B * (NC + 2), 0.f);
    for (auto& v : x) v = rnd();
    for (int b = 0; b < B; ++b) { if (b % 10 == 3) continue; t[b * (NC + 2) + (b * 5) % (NC - 1)] = 1.f; if (b % 4 == 0) t[b * (NC + 2) + (b * 3) % (NC - 1)] = 0.5f; }
    size_t ns; rgqa_maha_state_doubles(NC, H, &ns);
    std::vector<double> st(ns + 8, 0.0), st2(ns + 8, 0.0);
    for (int i = 0; i < 8; ++i) st[ns + i] = st2[ns + i] = 42.0;
    size_t sb; rgqa_maha_scratch_bytes(B, NC, &sb);
    std::vector<char> scratch(sb);
    if (rgqa_maha_accumulate(x.data(), H + 1, t.data(), NC + 2, B, H, NC, st.data(), scratch.data(), sb, nullptr)) return 100;
    int cut = B / 3;
    rgqa_maha_accumulate(x.data(), H + 1, t.data(), NC + 2, cut, H, NC, st2.data(), scratch.data(), sb, nullptr);
    rgqa_maha_accumulate(x.data() + (size_t)cut * (H + 1), H + 1, t.data() + (size_t)cut * (NC + 2), NC + 2, B - cut, H, NC, st2.data(), scratch.data(), sb, nullptr);
    int bad = 0;
    if (memcmp(st.data(), st2.data(), (ns + 8) * 8)) { printf("two batches differ from one\n"); ++bad; }
    for (int i = 0; i < 8; ++i) if (st[ns + i] != 42.0) { printf("state overrun\n"); ++bad; }
    for (int c = 0; c < NC; ++c) {
        double n = 0; std::vector<double> s(H, 0.0);
        for (int b = 0; b < B; ++b) if (t[b * (NC + 2) + c] != 0.f) { n += 1; for (int h = 0; h < H; ++h) s[h] += x[b * (H + 1) + h]; }
        if (st[c] != n) { printf("count mismatch c=%d\n", c); ++bad; }
        for (int h = 0; h < H; ++h) if (std::fabs(st[NC + (size_t)c * H + h] - s[h]) > 1e-12 * (std::fabs(s[h]) + 1)) { if (bad < 5) printf("sum mismatch c=%d h=%d\n", c, h); ++bad; }
    }
    const double* G = st.data() + NC + (size_t)NC * H;
    for (int i = 0; i < H; ++i) for (int j = 0; j < H; ++j) {
        double s = 0;
        for (int b = 0; b < B; ++b) { int k = 0; for (int c = 0; c < NC; ++c) k += t[b * (NC + 2) + c] != 0.f; s += (double)k * x[b * (H + 1) + i] * x[b * (H + 1) + j]; }
        if (std::fabs(G[i * H + j] - s) > 1e-12 * (std::fabs(s) + 1)) { if (bad < 5) printf("G mismatch %d %d got %g ref %g\n", i, j, G[i * H + j], s); ++bad; }
        if (G[i * H + j] != G[j * H + i]) ++bad;
    }
    printf("accumulate B=%d H=%d NC=%d: %d bad\n", B, H, NC, bad);
    return bad;
}
int main() {
    int bad = 0;
    bad += check_score(9, 40, 37, 50, true);       // T = 1 variant
    bad += check_score(35, 70, 66, 45, false);
    bad += check_dpooled(11, 70, 37, 23);
    bad += check_acc(300, 70, 37);
    // T = 2 variant: force it through a wide problem (>= 256 tiles of 32 x 32): 33 rows x 4100 classes
    bad += check_score(33, 8, 5, 4100, false);
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
