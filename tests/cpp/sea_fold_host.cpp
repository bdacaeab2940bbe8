// sea_fold_host.cpp -- the pre-folded SeaHash helpers of csrc/device_prelude.hpp (sea_tail_folded, sea_inner_folded, sea_order_lane_folded,
// sea_pair_folded: what the generated request-group kernel hashes with) against the unfolded forms every other path keeps using, on the HOST --
// the prelude's hash functions are __host__ __device__.  A stand-alone program, so that the host sanitizers can run it:
//   hipcc --offload-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//         tests/cpp/sea_fold_host.cpp -o tests/cpp/_build/sea_fold_host && tests/cpp/_build/sea_fold_host
// (tests/test_sea_fold_host.py builds and runs it that way.)  It touches no GPU.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define GGRS_SHARED_CODE(...) __VA_ARGS__
#include "../../bevy_ggrs_amd/csrc/device_prelude.hpp"
#undef GGRS_SHARED_CODE

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                                   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static unsigned long long n_checked = 0;
static void expect(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t c) {
    ++n_checked;
    if (!ok) { fprintf(stderr, "sea_fold_host: FAILED %s at inputs %016llx %016llx %016llx\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c); exit(1); }
}

// what SeaHasher makes of a spec of `nbytes` bytes: one full word, then the low nbytes - 8 bytes of `tail`
static uint64_t stream_finish(uint64_t full, uint64_t tail, uint32_t nbytes) {
    SeaStream st;
    st.write(full, 8);
    if (nbytes > 8) st.write(tail, nbytes - 8);
    return st.finish();
}

static void check(uint64_t full, uint64_t tail, uint64_t order) {
    // 9-, 12- and 16-byte specs: a full word and a tail of 1, 4 and 8 bytes.  The generated kernel memoises tails of <= 4 bytes; a 16-byte spec's second
    // word is a full word to SeaStream (finish xors 16 with no tail diffuse pending), which the folded form covers only as the PAIR below -- so the 16-byte
    // case here is the pair's own shape: write_u64(a); write_u64(b); finish()
    const uint64_t t1 = tail & 0xffull, t4 = tail & 0xffffffffull;
    expect(sea_inner_folded(full, sea_tail_folded(t1, 9)) == stream_finish(full, tail, 9), "9-byte spec", full, tail, 0);
    expect(sea_inner_folded(full, sea_tail_folded(t4, 12)) == stream_finish(full, tail, 12), "12-byte spec", full, tail, 0);
    expect(sea_inner_folded(full, sea_tail_folded(t4, 12)) == sea_inner3((uint32_t)full, (uint32_t)(full >> 32), (uint32_t)t4), "12-byte spec against sea_inner3", full, tail, 0);
    expect(sea_pair_folded(sea_order_lane_folded(full), tail) == stream_finish(full, tail, 16), "16-byte spec", full, tail, 0);
    // the pair: order index + inner hash
    const uint64_t inner = stream_finish(full, tail, 12);
    expect(sea_pair_folded(sea_order_lane_folded(order), inner) == sea_pair(order, inner), "pair against sea_pair", order, inner, 0);
    expect(sea_pair_folded(sea_order_lane_folded(order), inner) == sea_pair_pre(sea_order_lane(order), inner), "pair against sea_pair_pre", order, inner, 0);
    // the whole per-entity hash as the kernel spells it, against SeaStream end to end
    SeaStream p; p.write(order, 8); p.write(inner, 8);
    expect(sea_pair_folded(sea_order_lane_folded(order), sea_inner_folded(full, sea_tail_folded(t4, 12))) == p.finish(), "entity hash end to end", full, tail, order);
    // a memoised tail recomputed after its word changed is the fresh value: nothing of the old one survives
    uint64_t ma = sea_tail_folded(t4, 12);
    const uint64_t t4b = (uint32_t)(order ^ (order >> 32));
    if (t4b != t4) ma = sea_tail_folded(t4b, 12);
    expect(sea_inner_folded(full, ma) == stream_finish(full, t4b, 12), "recomputed tail", full, t4b, 0);
}

int main() {
    const uint64_t edge[] = {0ull, ~0ull, 1ull << 31, 1ull << 63, 0x80000000ull /* the bits of -0.0f */, 1ull, 0xffffffffull, 0xffffffff00000000ull};
    const int ne = (int)(sizeof edge / sizeof edge[0]);
    for (int i = 0; i < ne; ++i) for (int j = 0; j < ne; ++j) for (int k = 0; k < ne; ++k) check(edge[i], edge[j], edge[k]);
    for (int i = 0; i < 1000000; ++i) {
        const uint64_t a = rng(), b = rng(), c = rng();
        check(a, b, c);
        if ((i & 1023) == 0) for (int j = 0; j < ne; ++j) { check(edge[j], b, c); check(a, edge[j], c); check(a, b, edge[j]); }
    }
    printf("sea_fold_host: ok (%llu comparisons)\n", n_checked);
    return 0;
}
