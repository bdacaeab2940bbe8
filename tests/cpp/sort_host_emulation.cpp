// The sorted query's kernels (bevy_ggrs_amd/csrc/kernels.hpp: k_sort_rows / k_sort_rekey / k_sort_small / k_sort_emit, and the k_ix_* passes they are built on)
// executed on the HOST: their own text (IX_KERNELS_INC and SORT_KERNELS_INC, cut out of kernels.hpp by tests/test_sorted_query_model.py), one block at a time, one
// thread per lane, __syncthreads = a barrier, __ballot through shared memory, every array exactly as long as the launch may touch.  Compared with
// std::stable_sort over the transformed keys of the matching slots in slot order.  What the cut text needs from the rest of kernels.hpp -- the column addressing,
// the width-switched load and store, the query's argument block -- is restated here in its simplest form (one linear column per word).  So the tile-major addressing of
// the real col_at (col_ts, the 8192-slot layout tile) is NOT exercised here: the gathers through it are held by the buffer-exact GPU tests alone.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <thread>
#include <algorithm>
#include <pthread.h>
#include <random>
#include "ggrs_hip.h"
struct D3 { uint32_t x = 0, y = 0, z = 0; };
static thread_local D3 threadIdx; static D3 blockIdx, gridDim;
static pthread_barrier_t g_bar, g_wbar[16]; static uint8_t g_pred[1024]; static uint32_t g_val[1024];
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static void __syncthreads() { pthread_barrier_wait(&g_bar); }
static void __threadfence_block() { __sync_synchronize(); }
static void wave_sync() { pthread_barrier_wait(&g_wbar[threadIdx.x >> 6]); }
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
// ---- restated: one linear column per word (tile stride unused), loads and stores by width, the query's argument block and its batch
constexpr uint32_t TPB = 256, QUERY_BATCH = 4;
constexpr int MAX_COMPS = GGRS_MAX_COMPONENTS;
static uint64_t col_at(uint64_t col_off, uint32_t, uint32_t word_bytes, uint64_t e) { return col_off + e * word_bytes; }
static uint64_t diff_load(const uint8_t* p, uint32_t wb) { uint64_t v = 0; memcpy(&v, p, wb); return v; }
static void query_store(uint8_t* p, uint64_t v, uint32_t wb) { memcpy(p, &v, wb); }
struct QueryArgs {
    const uint8_t* state; uint8_t* out;
    uint64_t len, max_rows, off_alive, slots_off;
    uint64_t off_mask[MAX_COMPS];
    uint64_t col_off[GGRS_QUERY_MAX_WORDS];
    uint64_t out_off[GGRS_QUERY_MAX_WORDS];
    uint64_t* unit_match; uint64_t* unit_off;
    uint32_t col_ts[GGRS_QUERY_MAX_WORDS];
    uint32_t n_units, n_masks, without, n_words, slots;
    uint8_t col_wb[GGRS_QUERY_MAX_WORDS];
};
#include IX_KERNELS_INC
#include SORT_KERNELS_INC
template <typename F> void launch(uint32_t grid, uint32_t tpb, F f) {
    pthread_barrier_init(&g_bar, nullptr, tpb);
    for (uint32_t q = 0; q < tpb / 64; ++q) pthread_barrier_init(&g_wbar[q], nullptr, 64);
    gridDim.x = grid;
    for (uint32_t b = 0; b < grid; ++b) {
        blockIdx.x = b; memset(g_pred, 0, sizeof g_pred);
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < tpb; ++t) th.emplace_back([=] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
    pthread_barrier_destroy(&g_bar);
}
static uint64_t image(uint64_t v, uint32_t wb, uint32_t kind) {                 // the header's words, written independently of the kernels' text
    const uint32_t bits = 8 * wb; const uint64_t mask = bits == 64 ? ~0ull : (1ull << bits) - 1, sign = 1ull << (bits - 1);
    uint64_t t = v;
    if ((kind & 0xFF) == GGRS_SORT_I) t = v ^ sign;
    if ((kind & 0xFF) == GGRS_SORT_F) t = (v & sign) ? (~v & mask) : (v | sign);
    return (kind & GGRS_SORT_DESC) ? mask - t : t;
}
struct Key { uint32_t wb, kind, pat; };                                          // pat 0: random bits, 1: fewer than 8 distinct values
int main() {
    std::mt19937_64 rng(11);
    // n_matched and the keys sorted by at that size (a host thread per lane is slow: every size, width, kind and pattern is met once, not every combination)
    const std::vector<std::pair<uint64_t, std::vector<Key>>> plan = {
        {1, {{1, GGRS_SORT_U, 0}}}, {1, {{2, GGRS_SORT_I, 0}}},
        {65, {{4, GGRS_SORT_U | GGRS_SORT_DESC, 1}}}, {65, {{4, GGRS_SORT_F, 0}}},
        {2000, {{1, GGRS_SORT_I, 1}, {8, GGRS_SORT_U, 0}}},
        {2049, {{8, GGRS_SORT_I | GGRS_SORT_DESC, 0}}}, {2049, {{4, GGRS_SORT_F | GGRS_SORT_DESC, 1}, {2, GGRS_SORT_U, 1}}},
        {4100, {{8, GGRS_SORT_F, 0}}}, {4100, {{2, GGRS_SORT_I, 0}}}};
    int cases = 0;
    for (const auto& pc : plan) for (int form = 0; form < 2; ++form) {          // form 0: the large form, 1: k_sort_small
        const uint64_t n = pc.first; const std::vector<Key>& cfg = pc.second;
        if (form == 1 && n > IX_TILE) continue;
        // a state of len slots, about one slot in ten not matching, exactly n matching; one linear column per key word and one fetched u16 column
        std::vector<uint32_t> slots;
        uint64_t len = 0;
        while (slots.size() < n) { if (rng() % 10) slots.push_back((uint32_t)len); ++len; }
        const uint32_t n_units = (uint32_t)((len + 63) / 64);
        std::vector<uint64_t> unit_match(n_units + 1, 0), unit_off(n_units + 1, 0);
        for (uint32_t s : slots) unit_match[s >> 6] |= 1ull << (s & 63);
        for (uint32_t u = 0; u < n_units; ++u) unit_off[u + 1] = unit_off[u] + __builtin_popcountll(unit_match[u]);
        std::vector<uint64_t> col_start; uint64_t bytes = 0;
        for (const Key& k : cfg) { col_start.push_back(bytes); bytes += len * k.wb; }
        const uint64_t fetch_start = bytes; bytes += len * 2;
        std::vector<uint8_t> state(bytes);
        for (size_t q = 0; q < cfg.size(); ++q) for (uint64_t e = 0; e < len; ++e) {
            uint64_t v = cfg[q].pat ? (rng() % 5) * 0x8000000080000081ull : rng();
            memcpy(&state[col_start[q] + e * cfg[q].wb], &v, cfg[q].wb);
        }
        for (uint64_t e = 0; e < len; ++e) { const uint16_t v = (uint16_t)(e * 7 + 1); memcpy(&state[fetch_start + e * 2], &v, 2); }
        const uint64_t n_rows = std::min<uint64_t>(n, 1500);                     // a top-k below n where n is larger
        const uint64_t slots_off = (n_rows * 2 + 3) & ~3ull;                     // (the real layout aligns every column to 256 bytes)
        std::vector<uint8_t> out(slots_off + n_rows * 4);
        QueryArgs a; memset(&a, 0, sizeof a);
        a.state = state.data(); a.out = out.data(); a.len = len; a.max_rows = n_rows; a.slots_off = slots_off; a.col_off[0] = fetch_start; a.out_off[0] = 0;
        a.unit_match = unit_match.data(); a.unit_off = unit_off.data(); a.n_units = n_units; a.n_words = 1; a.slots = 1; a.col_wb[0] = 2;
        std::vector<uint32_t> key[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)}, val[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        const uint32_t n_tiles = (uint32_t)((n + IX_TILE - 1) / IX_TILE);
        std::vector<uint32_t> hist((size_t)n_tiles * 256);
        SortArgs s; memset(&s, 0, sizeof s);
        s.state = state.data(); s.n = n;
        for (int i = 0; i < 2; ++i) { s.key[i] = key[i].data(); s.val[i] = val[i].data(); }
        for (size_t q = cfg.size(); q-- > 0;) for (uint32_t half = 0; half < (cfg[q].wb == 8 ? 2u : 1u); ++half) {      // as the host stages them
            SortStage& st = s.st[s.n_stages++];
            st.col_off = col_start[q]; st.passes = cfg[q].wb >= 4 ? 4 : cfg[q].wb; st.wb = (uint8_t)cfg[q].wb;
            st.kind = (uint8_t)(cfg[q].kind & 0xFF); st.desc = (cfg[q].kind & GGRS_SORT_DESC) ? 1 : 0; st.half = (uint8_t)half;
        }
        const uint32_t grid = 1 + (uint32_t)(rng() % 3);                         // grid-stride launches: 1 .. 3 workgroups
        launch(grid, TPB, [=] { k_sort_rows(a, s); });
        uint32_t cur = 0;
        if (form == 1) { launch(1, IX_TPB, [=] { k_sort_small(s); }); for (uint32_t g = 0; g < s.n_stages; ++g) cur ^= s.st[g].passes & 1u; }
        else for (uint32_t g = 0; g < s.n_stages; ++g) {
            if (g) launch(grid, TPB, [=] { k_sort_rekey(s, g, cur); });
            for (uint32_t p = 0; p < s.st[g].passes; ++p, cur ^= 1u) {
                IxArgs x; memset(&x, 0, sizeof x);
                x.key_in = s.key[cur]; x.val_in = s.val[cur]; x.key_out = s.key[cur ^ 1u]; x.val_out = s.val[cur ^ 1u]; x.hist = hist.data();
                x.n = n; x.n_tiles = n_tiles; x.shift = 8 * p;
                launch(n_tiles, IX_TPB, [=] { k_ix_hist<false>(x); }); launch(1, IX_SCAN_TPB, [&] { k_ix_scan(hist.data(), n_tiles); }); launch(n_tiles, IX_TPB, [=] { k_ix_scatter<false>(x); });
            }
        }
        const uint32_t* perm = s.val[cur];
        launch(grid, TPB, [=] { k_sort_emit(a, perm, n_rows); });
        // the definition
        std::vector<uint32_t> want = slots;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
            for (size_t q = 0; q < cfg.size(); ++q) {
                uint64_t vx = 0, vy = 0; memcpy(&vx, &state[col_start[q] + (uint64_t)x * cfg[q].wb], cfg[q].wb); memcpy(&vy, &state[col_start[q] + (uint64_t)y * cfg[q].wb], cfg[q].wb);
                const uint64_t ix = image(vx, cfg[q].wb, cfg[q].kind), iy = image(vy, cfg[q].wb, cfg[q].kind);
                if (ix != iy) return ix < iy;
            }
            return false;
        });
        for (uint64_t r = 0; r < n_rows; ++r) {
            uint32_t got_slot; uint16_t got_word; memcpy(&got_slot, &out[slots_off + r * 4], 4); memcpy(&got_word, &out[r * 2], 2);
            if (got_slot != want[r] || got_word != (uint16_t)(want[r] * 7 + 1)) { printf("FAIL n=%llu form=%d keys=%zu row=%llu: slot %u vs %u\n", (unsigned long long)n, form, cfg.size(), (unsigned long long)r, got_slot, want[r]); return 1; }
        }
        ++cases;
    }
    printf("%d cases: the kernels' text equals the definition\n", cases);
    return 0;
}
