// driver of the host build of csrc/branched_loss.hip and csrc/conf_head.hip (kernels.h beside it), run by tests/test_branched_host.py:
//   emu DIR B NA NAp mce N
// reads DIR/z.bin [B, NA], c.bin [B], t.bin [B, NA + 1] (f32) and runs the loss operator; with N > 0 also x.bin, dg.bin [B, N], dconf.bin [B], gamma.bin,
// beta.bin, w3.bin [N], b3.bin [1] and runs the conf tail forward and backward (element type float).  Every operand sits in an allocation of exactly its
// size (a sanitizer build sees any access past it), outputs carry guard words; results go to DIR/<name>.out for the test to compare against torch.
#include "rgqa_amd/csrc/branched_loss.cpp"
#include "rgqa_amd/csrc/conf_head.cpp"
#include <string>

static std::string dir;
static std::vector<float> rd(const char* name, size_t n) {
    std::vector<float> v(n);
    FILE* f = fopen((dir + "/" + name + ".bin").c_str(), "rb");
    if (!f || fread(v.data(), 4, n, f) != n) { printf("cannot read %s\n", name); exit(2); }
    fclose(f);
    return v;
}
static void wr(const char* name, const void* p, size_t bytes) {
    FILE* f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { printf("cannot write %s\n", name); exit(2); }
    fclose(f);
}
static int guards(const std::vector<float>& v, size_t n, float g) { int bad = 0; for (size_t i = n; i < v.size(); ++i) bad += v[i] != g; return bad; }

int main(int argc, char** argv) {
    if (argc < 7) { printf("usage: emu DIR B NA NAp mce N\n"); return 2; }
    dir = argv[1];
    const int B = atoi(argv[2]), NA = atoi(argv[3]), NAp = atoi(argv[4]), mce = atoi(argv[5]), N = atoi(argv[6]);
    int bad = 0;
    {
        std::vector<float> z = rd("z", (size_t)B * NA), c = rd("c", B), t = rd("t", (size_t)B * (NA + 1));
        const size_t ns = k_branched_loss_scratch_floats(B);
        std::vector<float> scratch(ns + 4, 5.f), loss(3 + 2, 9.f), dl((size_t)B * NAp + 4, 7.f), dconf(B + 2, 9.f), conf(B + 2, 9.f), s1(B + 2, 9.f);
        std::vector<int64_t> label(B + 2, -5);
        if (k_branched_loss(z.data(), NA, c.data(), t.data(), NA + 1, B, NA, NAp, mce, 1.0f, loss.data(), dl.data(), NAp, dconf.data(), conf.data(), label.data(), s1.data(),
                            scratch.data(), nullptr)) return 3;
        bad += guards(scratch, ns, 5.f) + guards(loss, 3, 9.f) + guards(dl, (size_t)B * NAp, 7.f) + guards(dconf, B, 9.f) + guards(conf, B, 9.f) + guards(s1, B, 9.f);
        bad += (label[B] != -5) + (label[B + 1] != -5);
        // the same call without the loss and without dlogits (the engine's conf_only form): dconf keeps its bits
        std::vector<float> dconf2(B, 0.f);
        if (k_branched_loss(z.data(), NA, c.data(), t.data(), NA + 1, B, NA, NAp, mce, 1.0f, nullptr, nullptr, 0, dconf2.data(), nullptr, nullptr, nullptr, nullptr, nullptr)) return 3;
        bad += memcmp(dconf2.data(), dconf.data(), 4 * (size_t)B) != 0;
        wr("loss", loss.data(), 12); wr("dl", dl.data(), 4 * (size_t)B * NAp); wr("dconf_out", dconf.data(), 4 * (size_t)B); wr("conf", conf.data(), 4 * (size_t)B);
        wr("score1", s1.data(), 4 * (size_t)B); wr("label", label.data(), 8 * (size_t)B);
        float x[8] = {0};
        if (k_branched_loss(x, 4, x, x, 4, 1, 4, 4, 0, 1.f, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) { printf("a target without the UQ column accepted\n"); ++bad; }
        if (k_branched_loss(x, 4, x, x, 5, 1, 4, 4, 0, 1.f, x, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) { printf("loss without scratch accepted\n"); ++bad; }
    }
    if (N > 0) {
        std::vector<float> x = rd("x", (size_t)B * N), dg = rd("dg", (size_t)B * N), dconf = rd("dconf", B), gamma = rd("gamma", N), beta = rd("beta", N), w3 = rd("w3", N), b3 = rd("b3", 1);
        std::vector<float> cl(B + 2, 9.f), mean(B + 2, 9.f), rstd(B + 2, 9.f), gc((size_t)B * N + 4, 7.f), dgam(N + 2, 3.f), dbet(N + 2, 3.f), dw3(N + 2, 3.f), db3(1 + 2, 3.f);
        if (k_conf_tail_fwd<float>(x.data(), N, gamma.data(), beta.data(), w3.data(), b3.data(), cl.data(), mean.data(), rstd.data(), B, N, 1e-12f, nullptr)) return 3;
        if (k_conf_tail_bwd<float>(dconf.data(), x.data(), dg.data(), N, gamma.data(), beta.data(), w3.data(), mean.data(), rstd.data(), gc.data(), N, dgam.data(), dbet.data(),
                                   dw3.data(), db3.data(), 0, B, N, nullptr)) return 3;
        bad += guards(cl, B, 9.f) + guards(mean, B, 9.f) + guards(rstd, B, 9.f) + guards(gc, (size_t)B * N, 7.f) + guards(dgam, N, 3.f) + guards(dbet, N, 3.f) + guards(dw3, N, 3.f) + guards(db3, 1, 3.f);
        // accumulate = 1 on top of the first result doubles it exactly
        std::vector<float> a(dgam.begin(), dgam.begin() + N), d1(db3.begin(), db3.begin() + 1);
        if (k_conf_tail_bwd<float>(dconf.data(), x.data(), dg.data(), N, gamma.data(), beta.data(), w3.data(), mean.data(), rstd.data(), gc.data(), N, dgam.data(), dbet.data(),
                                   dw3.data(), db3.data(), 1, B, N, nullptr)) return 3;
        for (int j = 0; j < N; ++j) bad += dgam[j] != 2.f * a[j];
        bad += db3[0] != 2.f * d1[0];
        for (int j = 0; j < N; ++j) { dgam[j] *= 0.5f; dbet[j] *= 0.5f; dw3[j] *= 0.5f; }
        db3[0] *= 0.5f;
        wr("cl", cl.data(), 4 * (size_t)B); wr("gc", gc.data(), 4 * (size_t)B * N); wr("dgamma", dgam.data(), 4 * (size_t)N); wr("dbeta", dbet.data(), 4 * (size_t)N);
        wr("dw3", dw3.data(), 4 * (size_t)N); wr("db3", db3.data(), 4);
        std::vector<float> y(4, 0.f);
        if (k_conf_tail_fwd<float>(y.data(), 4, y.data(), y.data(), y.data(), y.data(), y.data(), y.data(), y.data(), 1, 4096, 1e-12f, nullptr) == 0) { printf("N = 4096 accepted\n"); ++bad; }
    }
    if (bad) printf("guard words overwritten / bit conditions broken (%d)\n", bad);
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
