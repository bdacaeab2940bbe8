// The build kernels of the peer index (bevy_ggrs_amd/csrc/kernels.hpp k_ix_*) executed on the HOST: their own text (IX_KERNELS_INC, cut out of kernels.hpp by
// tests/test_peer_index_model.py), one block at a time, one thread per lane, __syncthreads = a barrier, __ballot through shared memory, every array exactly as
// long as the launch may touch.  Compared with the definition: bucket k = the visible slots whose key is k, ascending.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <thread>
#include <algorithm>
#include <pthread.h>
#include <random>
struct D3 { uint32_t x = 0, y = 0, z = 0; };
static thread_local D3 threadIdx; static D3 blockIdx;
static pthread_barrier_t g_bar, g_wbar[16]; static uint8_t g_pred[1024]; static uint32_t g_val[1024];
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static void __syncthreads() { pthread_barrier_wait(&g_bar); }
static void __threadfence_block() { __sync_synchronize(); }
static void wave_sync() { pthread_barrier_wait(&g_wbar[threadIdx.x >> 6]); }          // what a wave does in lock-step: only its own 64 lanes meet
static uint64_t __ballot(bool p) {
    g_pred[threadIdx.x] = p; wave_sync();
    uint64_t m = 0; const uint32_t w0 = threadIdx.x & ~63u;
    for (uint32_t l = 0; l < 64; ++l) m |= (uint64_t)g_pred[w0 + l] << l;
    wave_sync(); return m;
}
static uint32_t shfl_from(uint32_t v, uint32_t src_lane) {
    g_val[threadIdx.x] = v; wave_sync();
    const uint32_t r = g_val[(threadIdx.x & ~63u) + (src_lane & 63u)];
    wave_sync(); return r;
}
static uint32_t __shfl(uint32_t v, uint32_t lane) { return shfl_from(v, lane); }
static uint32_t __shfl_xor(uint32_t v, uint32_t m) { return shfl_from(v, (threadIdx.x & 63u) ^ m); }
static uint32_t __shfl_up(uint32_t v, uint32_t d) { const uint32_t l = threadIdx.x & 63u; return shfl_from(v, l >= d ? l - d : l); }
static uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __sync_fetch_and_add(p, v); }
static int __popcll(uint64_t x) { return __builtin_popcountll(x); }
using std::min;
#include IX_KERNELS_INC
template <typename F> void launch(uint32_t grid, uint32_t tpb, F f) {
    pthread_barrier_init(&g_bar, nullptr, tpb);
    for (uint32_t q = 0; q < tpb / 64; ++q) pthread_barrier_init(&g_wbar[q], nullptr, 64);
    for (uint32_t b = 0; b < grid; ++b) {
        blockIdx.x = b; memset(g_pred, 0, sizeof g_pred);
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < tpb; ++t) th.emplace_back([=] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
    pthread_barrier_destroy(&g_bar);
}
int main() {
    std::mt19937_64 rng(7);
    const uint64_t sizes[] = {1, 2000, 2049, 8000};              // one lane; most of a tile; across the 2048-slot tile; four tiles
    const uint32_t buckets[] = {255, 300};                       // one radix pass and two
    int cases = 0;
    for (int small = 0; small < 2; ++small) for (uint64_t n : sizes) for (uint32_t nb : buckets) for (int pat = 0; pat < 3; ++pat) {      // the large form, then k_ix_small
        // exactly-sized heap arrays: a sanitizer sees any access beyond them
        std::vector<uint32_t> key(n), k0(n), k1(n), val(n), slots(n), start(nb + 1, 0xDEAD);
        std::vector<uint64_t> vis((n + 63) / 64, 0);
        for (uint64_t i = 0; i < n; ++i) {
            key[i] = pat == 0 ? (uint32_t)(rng() % (2ull * nb)) : pat == 1 ? nb / 2 : (uint32_t)rng();
            if (rng() % 10) vis[i >> 6] |= 1ull << (i & 63);
        }
        const uint32_t n_tiles = (uint32_t)((n + IX_TILE - 1) / IX_TILE), passes = nb <= 255 ? 1 : 2;
        std::vector<uint32_t> hist((size_t)n_tiles * 256);
        IxArgs pa[2]; memset(pa, 0, sizeof pa);
        for (uint32_t p = 0; p < passes; ++p) {
            IxArgs& a = pa[p];
            a.key_col = key.data(); a.vis = vis.data(); a.key_in = k0.data(); a.val_in = val.data();
            a.key_out = p == 0 ? k0.data() : k1.data(); a.val_out = p + 1 == passes ? slots.data() : val.data(); a.hist = hist.data();
            a.n = n; a.n_tiles = n_tiles; a.n_buckets = nb; a.shift = 8 * p;
            if (small) continue;
            if (p == 0) { launch(n_tiles, IX_TPB, [=] { k_ix_hist<true>(a); }); launch(1, IX_SCAN_TPB, [&] { k_ix_scan(hist.data(), n_tiles); }); launch(n_tiles, IX_TPB, [=] { k_ix_scatter<true>(a); }); }
            else { launch(n_tiles, IX_TPB, [=] { k_ix_hist<false>(a); }); launch(1, IX_SCAN_TPB, [&] { k_ix_scan(hist.data(), n_tiles); }); launch(n_tiles, IX_TPB, [=] { k_ix_scatter<false>(a); }); }
        }
        if (small && n_tiles > IX_SMALL_TILES) continue;          // (the host takes the large form there)
        if (small) { const IxArgs a0 = pa[0], a1 = pa[1]; launch(1, IX_TPB, [=] { k_ix_small(a0, a1, passes); }); }
        const uint32_t* sorted = passes == 1 ? k0.data() : k1.data();
        launch((nb + 1 + IX_TPB - 1) / IX_TPB, IX_TPB, [&] { k_ix_bounds(sorted, start.data(), n, nb); });
        // the definition
        std::vector<std::vector<uint32_t>> want(nb);
        for (uint64_t i = 0; i < n; ++i) if (((vis[i >> 6] >> (i & 63)) & 1) && key[i] < nb) want[key[i]].push_back((uint32_t)i);
        uint32_t at = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            if (start[b] != at) { printf("FAIL start n=%llu nb=%u pat=%d b=%u: %u vs %u\n", (unsigned long long)n, nb, pat, b, start[b], at); return 1; }
            for (uint32_t s : want[b]) { if (slots[at] != s) { printf("FAIL slot n=%llu nb=%u pat=%d\n", (unsigned long long)n, nb, pat); return 1; } ++at; }
        }
        if (start[nb] != at) { printf("FAIL total\n"); return 1; }
        ++cases;
    }
    printf("%d cases: the kernels' text equals the definition\n", cases);
    return 0;
}
