// driver of the host build of csrc/layer_taps.hip and csrc/conf_head.hip (kernels.h beside it), run by tests/test_layer_branched_host.py:
//   emu DIR taps B T X H varlen tail       gather + inject of the layer-wise confidence branch's tap points
//   emu DIR tail B N                       the conf tail forward and backward at a row width that is not 2 * hidden
// taps: reads DIR/src<i>.bin (f32 [rows_i, H]: rows_i = B for the last layer when tail = 1, else the language rows), lens.bin (int32 [B], varlen = 1), dtap.bin
// (f32 [X, B, H]), dy<i>.bin (f32, shaped like src<i>); writes taps.out [X, B, H], img.out (the bf16-image bytes of the rows read as split-f32 lines,
// [X, B, H * 2] bytes) and dy<i>.out.  Every operand sits in an allocation of exactly its size (a sanitizer build sees any access past it), outputs carry guard
// words; the test compares against numpy.
#include "rgqa_amd/csrc/layer_taps.cpp"
#include "rgqa_amd/csrc/conf_head.cpp"
#include <string>

static std::string dir;
template <typename U> static std::vector<U> rd(const std::string& name, size_t n) {
    std::vector<U> v(n);
    FILE* f = fopen((dir + "/" + name + ".bin").c_str(), "rb");
    if (!f || fread(v.data(), sizeof(U), n, f) != n) { printf("cannot read %s\n", name.c_str()); exit(2); }
    fclose(f);
    return v;
}
static void wr(const std::string& name, const void* p, size_t bytes) {
    FILE* f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { printf("cannot write %s\n", name.c_str()); exit(2); }
    fclose(f);
}
static int guards(const std::vector<float>& v, size_t n, float g) { int bad = 0; for (size_t i = n; i < v.size(); ++i) bad += v[i] != g; return bad; }
// 16-byte aligned storage of exactly n floats + 4 guard floats (operator new aligns to 16 on this platform; checked)
static std::vector<float> buf(size_t n, float g) { std::vector<float> v(n + 4, g); if (reinterpret_cast<uintptr_t>(v.data()) & 15) { printf("unaligned vector\n"); exit(2); } return v; }

static int run_taps(int B, int T, int X, int H, int varlen, int tail) {
    int bad = 0;
    std::vector<int> lens, cu;
    int rows = B * T;
    if (varlen) {
        lens = rd<int>("lens", B);
        cu.assign(B + 1, 0);
        for (int b = 0; b < B; ++b) cu[b + 1] = cu[b] + lens[b];
        rows = cu[B];
        cu.resize(B);            // the kernels read cu[b] for b < B only
    }
    const int* cup = varlen ? cu.data() : nullptr;
    std::vector<std::vector<float>> src(X), dy(X);
    TapSrcs ts; memset(&ts, 0, sizeof ts);
    for (int i = 0; i < X; ++i) {
        const bool compact = tail && i == X - 1;
        const size_t n = (size_t)(compact ? B : rows) * H;
        src[i] = rd<float>("src" + std::to_string(i), n);
        dy[i] = rd<float>("dy" + std::to_string(i), n);
        ts.p[i] = src[i].data(); ts.compact[i] = compact;
    }
    const size_t nt = (size_t)X * B * H;
    std::vector<float> taps = buf(nt, 7.f), img = buf(nt / 2, 5.f), dtap = rd<float>("dtap", nt);
    if (k_tap_gather(ts, X, B, cup, T, H * 4, taps.data(), img.data(), nullptr)) return 3;
    bad += guards(taps, nt, 7.f) + guards(img, nt / 2, 5.f);
    // without the image the copy keeps its bits
    std::vector<float> taps2 = buf(nt, 7.f);
    if (k_tap_gather(ts, X, B, cup, T, H * 4, taps2.data(), nullptr, nullptr)) return 3;
    bad += memcmp(taps.data(), taps2.data(), 4 * nt) != 0;
    for (int i = 0; i < X; ++i) {
        const bool compact = tail && i == X - 1;
        if (k_tap_inject<float>(dtap.data() + (size_t)i * B * H, H, dy[i].data(), H, compact ? nullptr : cup, compact ? 1 : T, B, H, nullptr)) return 3;
        wr("dy" + std::to_string(i), dy[i].data(), 4 * dy[i].size());
    }
    wr("taps", taps.data(), 4 * nt); wr("img", img.data(), 2 * nt);
    float x[8] = {0};
    TapSrcs t1; memset(&t1, 0, sizeof t1); t1.p[0] = x;
    if (k_tap_gather(t1, 1, 1, nullptr, 1, 24, x, nullptr, nullptr) == 0) { printf("rows of 24 bytes accepted\n"); ++bad; }
    if (k_tap_gather(t1, TAP_MAX_LAYERS + 1, 1, nullptr, 1, 16, x, nullptr, nullptr) == 0) { printf("too many layers accepted\n"); ++bad; }
    if (k_tap_gather(t1, 1, 1, nullptr, 1, 16, x, x, nullptr) == 0) { printf("an image of rows that are no whole lines accepted\n"); ++bad; }
    if (k_tap_inject<float>(x, 4, x, 4, nullptr, 1, 1, 4, nullptr) == 0) { printf("inject of 4 columns accepted\n"); ++bad; }
    return bad;
}

static int run_tail(int B, int N) {
    int bad = 0;
    std::vector<float> x = rd<float>("x", (size_t)B * N), dg = rd<float>("dg", (size_t)B * N), dconf = rd<float>("dconf", B), gamma = rd<float>("gamma", N), beta = rd<float>("beta", N),
                       w3 = rd<float>("w3", N), b3 = rd<float>("b3", 1);
    std::vector<float> cl(B + 2, 9.f), mean(B + 2, 9.f), rstd(B + 2, 9.f), gc((size_t)B * N + 4, 7.f), dgam(N + 2, 3.f), dbet(N + 2, 3.f), dw3(N + 2, 3.f), db3(1 + 2, 3.f);
    if (k_conf_tail_fwd<float>(x.data(), N, gamma.data(), beta.data(), w3.data(), b3.data(), cl.data(), mean.data(), rstd.data(), B, N, 1e-12f, nullptr)) return 3;
    if (k_conf_tail_bwd<float>(dconf.data(), x.data(), dg.data(), N, gamma.data(), beta.data(), w3.data(), mean.data(), rstd.data(), gc.data(), N, dgam.data(), dbet.data(),
                               dw3.data(), db3.data(), 0, B, N, nullptr)) return 3;
    bad += guards(cl, B, 9.f) + guards(mean, B, 9.f) + guards(rstd, B, 9.f) + guards(gc, (size_t)B * N, 7.f) + guards(dgam, N, 3.f) + guards(dbet, N, 3.f) + guards(dw3, N, 3.f) + guards(db3, 1, 3.f);
    wr("cl", cl.data(), 4 * (size_t)B); wr("gc", gc.data(), 4 * (size_t)B * N); wr("dgamma", dgam.data(), 4 * (size_t)N); wr("dbeta", dbet.data(), 4 * (size_t)N);
    wr("dw3", dw3.data(), 4 * (size_t)N); wr("db3", db3.data(), 4);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: emu DIR taps B T X H varlen tail | emu DIR tail B N\n"); return 2; }
    dir = argv[1];
    int bad = 0;
    if (std::string(argv[2]) == "taps" && argc == 9) bad = run_taps(atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]));
    else if (std::string(argv[2]) == "tail" && argc == 5) bad = run_tail(atoi(argv[3]), atoi(argv[4]));
    else { printf("bad arguments\n"); return 2; }
    if (bad) printf("guard words overwritten / bit conditions broken (%d)\n", bad);
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
