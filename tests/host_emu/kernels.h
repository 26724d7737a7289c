// Host stand-in for csrc/kernels.h (tests/host_emu/__init__.py build()): the "one workgroup per row" units of csrc/ compiled by the host compiler, every
// workgroup run as 256 std::threads with barriers for __syncthreads and per-wave barriers for __shfl_xor.  Checks indexing, bounds, the reductions and
// the arithmetic of the kernels where there is no GPU; a 16-byte access to an address that is not 16-byte aligned aborts.  It says nothing about speed.
// The row primitives and element formulas are csrc/rowops.h itself (with expf for __expf), copied beside this file by build().
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include <algorithm>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
inline thread_local dim3 threadIdx, blockIdx, gridDim, blockDim;
typedef void* hipStream_t;
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
#define __expf expf
inline std::barrier<>* g_block_bar;
inline std::barrier<>* g_wave_bar[4];
#define __syncthreads() g_block_bar->arrive_and_wait()
template <class T> T __shfl_xor(T v, int o, int width = 64) {
    static T buf[256];
    (void)width;
    const int t = threadIdx.x, w = t >> 6;
    buf[t] = v;
    g_wave_bar[w]->arrive_and_wait();
    T r = buf[(t & ~63) | ((t & 63) ^ o)];
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
using std::min; using std::isfinite;
inline float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
inline float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64)); return v; }
inline void need16(const void* p) { if (reinterpret_cast<uintptr_t>(p) & 15) { printf("16-byte access to a misaligned address\n"); abort(); } }
inline void load4(const float* p, float v[4]) { need16(p); memcpy(v, p, 16); }
inline void store4(float* p, const float v[4]) { need16(p); memcpy(p, v, 16); }
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
// the engine's other element types: distinct host types so that the units' explicit instantiations stay distinct (only float is run here)
struct bf16_t { float v; };
struct sf32 { float v; };
inline float ld_elem(const float* p) { return *p; }
inline float ld_elem(const bf16_t* p) { return p->v; }
inline float ld_elem(const sf32* p) { return p->v; }
inline void st_elem(float* p, float x) { *p = x; }
inline void st_elem(bf16_t* p, float x) { p->v = x; }
inline void st_elem(sf32* p, float x) { p->v = x; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
#include "rowops.h"
#define RGQA_OK 0
#define RGQA_ERR_ARG (-1)
#define RGQA_REQUIRE(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return RGQA_ERR_ARG; } } while (0)
#define RGQA_LAUNCH_CHECK(name) do { } while (0)
struct EnergyLossCfg { int mce; float weight, m_in, m_out; };
template <class K, class... A> void launch(K k, dim3 grid, dim3 block, A... args) {
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bb(block.x), w0(64), w1(64), w2(64), w3(64);
            g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(bx, by); gridDim = grid; blockDim = block; k(args...); g_block_bar->arrive_and_drop(); });
            for (auto& x : th) x.join();
        }
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) launch(k, grid, block, __VA_ARGS__)
