// sea_mad3_host.cpp -- the three-product multiply of csrc/device_prelude.hpp (sea_mul_p_mad3: what the generated kernel's hot path multiplies by SEA_P
// with on the device) against x * SEA_P, and the hot diffuse built on it against sea_diffuse, on the HOST.  The prelude's host build spells the hot multiply
// x * SEA_P; this program asks for the device's C expression instead (GGRS_SEA_MUL_HOT below), without its register constraint: GGRS_VGPR_OPAQUE is an empty
// asm on the device and has no meaning here.  A stand-alone program, so that the host sanitizers can run it:
//   hipcc --offload-host-only -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//         tests/cpp/sea_mad3_host.cpp -o tests/cpp/_build/sea_mad3_host && tests/cpp/_build/sea_mad3_host
// (tests/test_sea_mad3_host.py builds and runs it that way.)  It touches no GPU.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define GGRS_VGPR_OPAQUE(c) ((void)0)
#define GGRS_SEA_MUL_HOT(x) sea_mul_p_mad3(x)
#define GGRS_SHARED_CODE(...) __VA_ARGS__
#include "../../bevy_ggrs_amd/csrc/device_prelude.hpp"
#undef GGRS_SHARED_CODE

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rng() {                                   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static unsigned long long n_checked = 0;
static void expect(bool ok, const char* what, uint64_t x) {
    ++n_checked;
    if (!ok) { fprintf(stderr, "sea_mad3_host: FAILED %s at input %016llx\n", what, (unsigned long long)x); exit(1); }
}

static void check(uint64_t x) {
    expect(sea_mul_p_mad3(x) == x * SEA_P, "sea_mul_p_mad3 against x * SEA_P", x);
    expect(sea_diffuse_hot(x) == sea_diffuse(x), "sea_diffuse_hot against sea_diffuse", x);
    // the two helpers the hot diffuse serves, against the unfolded forms every other path keeps (plain sea_diffuse throughout)
    const uint32_t z = (uint32_t)(x ^ (x >> 29));
    expect(sea_inner_folded(x, sea_tail_folded(z, 12)) == sea_inner3((uint32_t)x, (uint32_t)(x >> 32), z), "sea_inner_folded against sea_inner3", x);
    expect(sea_pair_folded(sea_order_lane_folded(~x), x) == sea_pair(~x, x), "sea_pair_folded against sea_pair", x);
}

int main() {
    const uint64_t edge[] = {0ull, 1ull, 0xffffffffull /* 2^32 - 1: the low half at all-ones */, 1ull << 32, ~0ull, 0xffffffff00000000ull /* the high half at all-ones */};
    for (uint64_t e : edge) check(e);
    for (int b = 0; b < 64; ++b) check(1ull << b);
    for (int i = 0; i < 4096; ++i) check(rng());
    printf("sea_mad3_host: ok (%llu comparisons)\n", n_checked);
    return 0;
}
