// ubench_alu.hip -- the chip's ceiling for the checksum arithmetic: SeaHash `diffuse` (two 64-bit multiplies by a constant +
// a variable shift-xor) per second over all CUs, and the instruction mix behind it (v_mul_lo_u32 / v_mad_u64_u32 / v_fma_f32 chains).
// Used to state a roofline for the checksum-only paths (BASELINE config 5 after dead-snapshot elimination) and to judge how
// far the hash ALU of a fused tick is from its floor.   build: hipcc --offload-arch=gfx950 -O3 ubench_alu.hip -o ubench_alu
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
constexpr uint64_t P = 0x6eed0e9da4d94a4fULL;
// the kernels' own spelling (bevy_ggrs_amd/csrc/device_prelude.hpp sea_diffuse): the variable shift in 32-bit terms -- a ceiling measured with the 64-bit form
// (v_lshrrev_b64 per diffuse: rounds 4-5) was one the kernels could exceed (config 5 read 1.02 of it in profiles/r06final)
__device__ __forceinline__ uint64_t diffuse(uint64_t x) { x *= P; const uint32_t hi = (uint32_t)(x >> 32); x ^= (uint64_t)(hi >> (hi >> 28)); x *= P; return x; }

// EXPERIMENT (profiles/valu_trim): the multiply by P as three v_mad_u64_u32 and one add instead of what the compiler makes of `x *= P`
// (2 v_mul_lo_u32 + v_mad_u64_u32 + v_add3_u32).  The cross terms xh*Pl + xl*Ph go through a chain of two of them of which only the low half is
// used; the third is the full xl*Pl.  gfx950's VOP3 takes no literal: the halves of P sit in SGPRs.  v_mad_u64_u32 writes a carry-out: vcc, declared.
__device__ __forceinline__ uint64_t mad64_0(uint32_t a, uint32_t b) { uint64_t d; asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(d) : "v"(a), "s"(b) : "vcc"); return d; }
__device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) { uint64_t d; asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c) : "vcc"); return d; }
__device__ __forceinline__ uint64_t mul_p_mad3(uint64_t x) {
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32), pl = (uint32_t)P, ph = (uint32_t)(P >> 32);
    const uint64_t cross = mad64(xl, ph, mad64_0(xh, pl));         // low half: (xh*Pl + xl*Ph) mod 2^32; the high half is never read
    const uint64_t r = mad64_0(xl, pl);
    return r + ((uint64_t)(uint32_t)cross << 32);                    // one v_add_u32 on the high half
}
__device__ __forceinline__ uint64_t diffuse_mad3(uint64_t x) { x = mul_p_mad3(x); const uint32_t hi = (uint32_t)(x >> 32); x ^= (uint64_t)(hi >> (hi >> 28)); x = mul_p_mad3(x); return x; }

// ADOPTED (profiles/mad3_multiply): the same three products in plain C, as bevy_ggrs_amd/csrc/device_prelude.hpp sea_mul_p_mad3 spells them -- no instruction inside
// an asm statement (the compiler folds constants through it and allocates the temporaries itself); the empty asm only keeps it from narrowing the cross sum,
// of which the low half alone is used, back to v_mul_lo_u32
__device__ __forceinline__ uint64_t mul_p_c3(uint64_t x) {
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    uint64_t c = (uint64_t)xh * (uint32_t)P;
    c = (uint64_t)xl * (uint32_t)(P >> 32) + c;
    asm("" : "+v"(c));
    return (uint64_t)xl * (uint32_t)P + (c << 32);
}
__device__ __forceinline__ uint64_t diffuse_c3(uint64_t x) { x = mul_p_c3(x); const uint32_t hi = (uint32_t)(x >> 32); x ^= (uint64_t)(hi >> (hi >> 28)); x = mul_p_c3(x); return x; }

// MAD3: 0 = the compiler's lowering of x *= P, 1 = three mads through inline asm, 2 = three mads in plain C
template <int CH, int MAD3 = 0>
__global__ __launch_bounds__(256) void k_diffuse(uint64_t* out, int iters) {
    uint64_t x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = (uint64_t)(blockIdx.x * 256 + threadIdx.x) * 0x9e3779b97f4a7c15ull + c;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CH; ++c) x[c] = MAD3 == 2 ? diffuse_c3(x[c] ^ (uint64_t)i) : MAD3 == 1 ? diffuse_mad3(x[c] ^ (uint64_t)i) : diffuse(x[c] ^ (uint64_t)i);
    }
    uint64_t r = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) r ^= x[c];
    if (r == 0x1234567) out[0] = r;          // never true: keeps the chains alive
}
// the three spellings agree: one diffuse of each per thread, compared on the host
__global__ void k_diffuse_check(const uint64_t* in, uint64_t* a, uint64_t* b, uint64_t* c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = diffuse(in[i]); b[i] = diffuse_mad3(in[i]); c[i] = diffuse_c3(in[i]); }
}
template <int CH>
__global__ __launch_bounds__(256) void k_mad64(uint64_t* out, int iters) {           // v_mad_u64_u32 chains: x = lo(x) * K + x
    uint64_t x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = (uint64_t)(blockIdx.x * 256 + threadIdx.x) * 0x9e3779b97f4a7c15ull + c;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CH; ++c) x[c] = mad64((uint32_t)x[c], 0xa4d94a4fu, x[c]);
    }
    uint64_t r = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) r ^= x[c];
    if (r == 0x1234567) out[0] = r;
}
template <int CH>
__global__ __launch_bounds__(256) void k_mul32(uint32_t* out, int iters) {           // v_mul_lo_u32 chains
    uint32_t x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + c;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CH; ++c) x[c] = x[c] * 0xa4d94a4fu + (uint32_t)i;
    }
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) r ^= x[c];
    if (r == 0x1234567) out[0] = r;
}
template <int CH>
__global__ __launch_bounds__(256) void k_fma32(float* out, int iters) {              // v_fma_f32 chains (the full-rate reference)
    float x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = (float)(threadIdx.x + c);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CH; ++c) x[c] = __builtin_fmaf(x[c], 1.0000001f, 0.5f);
    }
    float r = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) r += x[c];
    if (r == 0.1234f) out[0] = r;
}

template <class F>
double time_ms(F launch) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    launch(); hipDeviceSynchronize();
    hipEventRecord(a); for (int i = 0; i < 5; ++i) launch(); hipEventRecord(b); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    return ms / 5;
}
int main() {
    int n_cu = 0; hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, 0);
    int clk = 0; hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, 0);
    void* out; hipMalloc(&out, 4096);
    const int iters = 4096;
    {   // the experiment's spelling against the kernels' own, on edge values and a few thousand others
        const int n = 4096; std::vector<uint64_t> h(n), ha(n), hb(n), hc(n);
        uint64_t z = 0x243f6a8885a308d3ull;
        for (int i = 0; i < n; ++i) { z = z * 6364136223846793005ull + 1442695040888963407ull; h[i] = z; }
        h[0] = 0; h[1] = ~0ull; h[2] = 1ull << 31; h[3] = 1ull << 63; h[4] = 0x80000000ull; h[5] = 0xffffffffull; h[6] = 0xffffffff00000000ull; h[7] = 1ull; h[8] = 1ull << 32;
        uint64_t *di, *da, *db, *dc; hipMalloc(&di, n * 8); hipMalloc(&da, n * 8); hipMalloc(&db, n * 8); hipMalloc(&dc, n * 8);
        hipMemcpy(di, h.data(), n * 8, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_diffuse_check, dim3(n / 256), dim3(256), 0, 0, di, da, db, dc, n);
        hipMemcpy(ha.data(), da, n * 8, hipMemcpyDeviceToHost); hipMemcpy(hb.data(), db, n * 8, hipMemcpyDeviceToHost); hipMemcpy(hc.data(), dc, n * 8, hipMemcpyDeviceToHost);
        int bad = 0; for (int i = 0; i < n; ++i) bad += ha[i] != hb[i] || ha[i] != hc[i];
        printf("mad3 spellings (asm, C) == own spelling on %d inputs: %s\n", n, bad ? "NO" : "yes");
        hipFree(di); hipFree(da); hipFree(db); hipFree(dc);
        if (bad) return 1;
    }
    printf("CUs %d, clock attr %d kHz\n", n_cu, clk);
    printf("%-28s %8s %12s %14s %14s\n", "kernel", "waves/SIMD", "ms", "G ops/s", "cyc/op/SIMD@2.4GHz");
    for (int wps : {1, 2, 4, 8}) {
        const int blocks = n_cu * wps;          // 256-thread blocks = 4 waves = 1 per SIMD
        auto report = [&](const char* name, double ms, double ops_per_thread) {
            const double ops = (double)blocks * 256 * ops_per_thread;     // lane-ops
            const double wave_ops_per_simd = ops / 64 / (n_cu * 4);
            printf("%-28s %8d %12.4f %14.1f %14.2f\n", name, wps, ms, ops / ms / 1e6, ms * 1e-3 * 2.4e9 / wave_ops_per_simd);
        };
        report("diffuse x1 chain", time_ms([&] { hipLaunchKernelGGL(k_diffuse<1>, dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 1.0);
        report("diffuse x4 chains", time_ms([&] { hipLaunchKernelGGL(k_diffuse<4>, dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 4.0);
        report("diffuse x8 chains", time_ms([&] { hipLaunchKernelGGL(k_diffuse<8>, dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 8.0);
        report("v_mul_lo_u32 x8 chains", time_ms([&] { hipLaunchKernelGGL(k_mul32<8>, dim3(blocks), dim3(256), 0, 0, (uint32_t*)out, iters); }), iters * 8.0);
        report("v_mad_u64_u32 x8 chains", time_ms([&] { hipLaunchKernelGGL(k_mad64<8>, dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 8.0);
        // the experiment, in the same process: the own spelling three more times (its spread is the bar), the mad3 spelling three times, interleaved
        for (int rep = 0; rep < 3; ++rep) {
            report("diffuse x8 chains (rep)", time_ms([&] { hipLaunchKernelGGL((k_diffuse<8, 0>), dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 8.0);
            report("mad3 diffuse x8 chains", time_ms([&] { hipLaunchKernelGGL((k_diffuse<8, 1>), dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 8.0);
            report("mad3-C diffuse x8 chains", time_ms([&] { hipLaunchKernelGGL((k_diffuse<8, 2>), dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 8.0);
        }
        report("mad3 diffuse x4 chains", time_ms([&] { hipLaunchKernelGGL((k_diffuse<4, 1>), dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 4.0);
        report("mad3-C diffuse x4 chains", time_ms([&] { hipLaunchKernelGGL((k_diffuse<4, 2>), dim3(blocks), dim3(256), 0, 0, (uint64_t*)out, iters); }), iters * 4.0);
        report("v_fma_f32 x8 chains", time_ms([&] { hipLaunchKernelGGL(k_fma32<8>, dim3(blocks), dim3(256), 0, 0, (float*)out, iters); }), iters * 8.0);
    }
    return 0;
}
