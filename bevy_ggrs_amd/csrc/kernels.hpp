// kernels.hpp -- gfx950 (CDNA4, wave64) device code of the rollback re-simulation engine.
//
// Everything here is HBM-bound element-wise integer/f32 work over SoA word columns: no MFMA
// (there is no contraction anywhere on this path).  Design rules applied:
//   * one workgroup (256 threads = 4 waves) owns one TILE of 1024 consecutive slots in EVERY
//     kernel, and tile t is always blockIdx t.  Workgroup b lands on XCD b % 8, so the same
//     XCD (and its private 4 MiB L2) touches the same slots in load -> advance -> save chains;
//   * word columns are stored TILE-MAJOR inside a state block, in LAYOUT TILES of 8192 slots (= 8 workgroup tiles): the
//     8192 slots of layout tile T of every registered word sit next to each other (tile_stride = bytes of all words of
//     8192 slots, 480 KiB for the particles world);
//     word w of slot e lives at  col_off[w] + (e >> 13) * tile_stride + (e & 8191) * word_bytes.
//     A workgroup's 1024-slot tile t is sub-tile t & 7 of layout tile t >> 3: its 4 KiB row of a 4-byte word starts at
//     col_off[w] + (t >> 3) * tile_stride + (t & 7) * 4096, and CONSECUTIVE ROWS OF ONE WORKGROUP ARE 32 KiB APART --
//     the period of the HBM channel interleave (128 channels x 256 B), so the rows a wave stores back to back land in
//     the same DRAM pages (scripts/ubench3.hip, layout 2 / G = 8: 100.6 us vs 108.5 us for 1024-slot layout tiles).
//     Live-only side columns keep the same formula with tile_stride = 8192 * word_bytes (a plain array);
//   * every column access is 16 B per lane (dwordx4), 1 KiB per wave instruction, all loads
//     of a tile issued before the first store;
//   * Rollback-entity liveness is a 1 bit/slot mask; despawn masks are built with wave64
//     __ballot and a scalar bit-interleave, live counts with popcount;
//   * f32 integration uses explicit __fmul_rn/__fadd_rn: Rust never contracts a*b+c, and the
//     checksum hashes the raw f32 bits, so results must be bit-exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ggrs {

constexpr int TILE = 1024;     // slots per workgroup
// LT_SHIFT = 13 / LAYOUT_TILE = 8192 (slots of a LAYOUT tile = 8 workgroup tiles) are declared in device_prelude.hpp
constexpr int TPB = 256;       // threads per workgroup (4 waves of 64)
constexpr int MAX_ROWS = 128;  // 4 KiB copy rows per tile (a 4-byte column = 1 row, 8-byte = 2): 64 eight-byte words
constexpr int MAX_COMPS = GGRS_MAX_COMPONENTS;
constexpr int MAX_MASKS = MAX_COMPS + 1;  // alive + one presence mask per component
constexpr int MAX_UNITS = 32;

// SeaHash (seahash 4.1), the state-block Header, wave_xor and the box_game step: shared with the run-time generated kernels
#define GGRS_SHARED_CODE(...) __VA_ARGS__
#include "device_prelude.hpp"
#undef GGRS_SHARED_CODE

// byte offset (inside a state block) of word-column element `e`: see the layout note at the top
__host__ __device__ __forceinline__ uint64_t col_at(uint64_t col_off, uint32_t tile_stride, uint32_t word_bytes, uint64_t e) {
    return col_off + (e >> LT_SHIFT) * (uint64_t)tile_stride + (e & (uint64_t)(LAYOUT_TILE - 1)) * (uint64_t)word_bytes;
}
// byte offset (relative to the column's col_off) of the first element of workgroup tile t (1024 slots)
__host__ __device__ __forceinline__ uint64_t wtile_off(uint32_t t, uint32_t tile_stride, uint32_t word_bytes) {
    return (uint64_t)(t >> (LT_SHIFT - 10)) * tile_stride + (uint64_t)(t & ((LAYOUT_TILE / TILE) - 1u)) * (uint32_t)(TILE * word_bytes);
}

// ------------------------------------------------------------------ kernel argument blocks
struct RowDesc {          // one 4 KiB-per-tile copy row of the packed state block
    uint64_t col_off;     // byte offset of the column inside the state block
    uint32_t roff;        // byte offset of this row inside the column's tile (0 or 4096)
    uint32_t tile_stride; // bytes one tile of this column spans (TILE * word_bytes)
    uint32_t word_bytes;
    uint32_t bytes;       // bytes of this row per workgroup tile: 4096, or 1024 / 2048 for a 1- / 2-byte word
};
struct CopyPlan {
    uint32_t n_rows, n_masks, n_wide, pad;   // rows [0, n_wide) are 4096-byte rows (moved in straight-line batches), the rest are short
    uint64_t mask_off[MAX_MASKS];
    RowDesc row[MAX_ROWS];
};
struct StepArgs {         // fused GgrsSchedule step of the particles workload
    uint8_t* state;
    uint64_t off_alive, off_pT, off_pV, off_pL;
    uint64_t off_t[3], off_v[3], off_ttl;
    uint32_t dt_bits; float g[3];
    uint64_t* part_T; uint64_t* part_V; uint64_t* part_cnt;
    uint32_t ts; uint32_t pad;            // tile stride of the rollback word columns
};

struct UnitDesc { uint64_t off; uint32_t wb; uint32_t ts; };   // one hashed word: slot e's word of wb bytes at col_at(off, ts, wb, e)
struct CksArgs {          // generic component checksum
    const uint8_t* state;
    uint64_t off_alive;
    uint32_t n_cks; uint32_t part_stride;
    uint64_t off_present[MAX_COMPS];
    uint32_t n_units[MAX_COMPS];
    uint32_t unit_base[MAX_COMPS];
    uint64_t* parts;      // [n_cks][part_stride]
    uint64_t* part_cnt;   // [part_stride]
};

// ------------------------------------------------------------------ helpers
// bit i of x (16 bits) -> bit 4*i
__device__ __forceinline__ uint64_t spread4(uint64_t x) {
    x &= 0xFFFFULL;
    x = (x | (x << 24)) & 0x000000FF000000FFULL;
    x = (x | (x << 12)) & 0x000F000F000F000FULL;
    x = (x | (x << 6)) & 0x0303030303030303ULL;
    x = (x | (x << 3)) & 0x1111111111111111ULL;
    return x;
}

// ------------------------------------------------------------------ finalize (device function)
// Hash each component's XOR once more (component_checksum.rs:92-95), add the entity part
// (entity_checksum.rs:29-52), XOR-fold all parts (checksum.rs:88-99).  Runs inside workgroup 0
// of the SaveWorld copy kernel (the partials were completed by the previous kernel on the
// stream), so a SaveWorld is ONE launch.
struct FinalizeArgs {
    const uint64_t* parts;      // [n_cks][part_stride]
    const uint64_t* part_cnt;   // [part_stride]
    uint32_t n_cks, part_stride, n_parts, enabled;
    uint64_t total_len;
    uint64_t* out;              // {lo, hi} of Checksum(u128)
    Header* live_hdr;
};
constexpr int MAX_CKS = MAX_COMPS;

__device__ __forceinline__ void finalize_block(const FinalizeArgs& f, uint64_t* checksum_out) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ uint64_t fin_sx[MAX_CKS + 1];
    // one partial column per wave at a time (wave-uniform control flow, loads pipelined)
    for (uint32_t k = wave; k <= f.n_cks; k += 4) {
        const bool is_cnt = (k == f.n_cks);
        const uint64_t* __restrict__ p = is_cnt ? f.part_cnt : f.parts + (uint64_t)k * f.part_stride;
        uint64_t x = 0, sum = 0;
#pragma unroll 8
        for (uint32_t i = lane; i < f.n_parts; i += 64) { const uint64_t v = p[i]; x ^= v; sum += v; }
        x = wave_xor(x);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) fin_sx[k] = is_cnt ? sum : x;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
        for (uint32_t k = 0; k < f.n_cks; ++k) total ^= sea_one(fin_sx[k]);
        const uint64_t active = fin_sx[f.n_cks];
        total ^= sea_pair(active, f.total_len);      // hash(active, total): same shape as pair()
        f.out[0] = total; f.out[1] = 0;              // `as u128` of a u64: upper half always 0
        f.live_hdr->active = active;
        f.live_hdr->checksum[0] = total; f.live_hdr->checksum[1] = 0;
        checksum_out[0] = total; checksum_out[1] = active;
    }
}

// ------------------------------------------------------------------ k_copy_state
// SaveWorld's Snapshot set (component_snapshot.rs:66-84, entity.rs:39-51, ring push
// mod.rs:147-181) and LoadWorld's Entity+Data sets (entity.rs:55-99,
// component_snapshot.rs:95-123, ring rollback mod.rs:210-226) both reduce to: copy every
// registered word column over [0, len) plus the liveness/presence masks between the live
// block and a ring slot.  Algorithmic traffic: 2 x (bytes per slot) per entity.
//
// Full tiles take a branch-free path: rows are moved in straight-line batches of 8/4/2/1
// (every load of a batch in flight before its first store -- a per-lane predicate around a
// load makes hipcc drain vmcnt after every single load).  Only the last, ragged tile uses the
// predicated path.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int B, bool NT>
__device__ __forceinline__ void copy_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                          const CopyPlan& plan, uint32_t r0, uint32_t t, uint32_t tid) {
    u32x4 v[B];
    uint64_t pos[B];
#pragma unroll
    for (int j = 0; j < B; ++j) {
        const RowDesc rd = plan.row[r0 + j];
        pos[j] = rd.col_off + wtile_off(t, rd.tile_stride, rd.word_bytes) + rd.roff + (uint64_t)tid * 16;
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (NT) v[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + pos[j]));
        else v[j] = *reinterpret_cast<const u32x4*>(src + pos[j]);
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (NT) __builtin_nontemporal_store(v[j], reinterpret_cast<u32x4*>(dst + pos[j]));
        else *reinterpret_cast<u32x4*>(dst + pos[j]) = v[j];
    }
}

template <bool NT>
__global__ __launch_bounds__(TPB) void k_copy_state(const uint8_t* __restrict__ src,
                                                    uint8_t* __restrict__ dst, CopyPlan plan,
                                                    uint64_t len, Header hdr, FinalizeArgs fin) {
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    __shared__ uint64_t cks[2];
    if (t == 0 && fin.enabled) finalize_block(fin, cks);       // workgroup-uniform branch

    const uint32_t n_rows = plan.n_rows;
    if (((uint64_t)t + 1) * TILE <= len) {
        const uint32_t n_wide = plan.n_wide;
        uint32_t r = 0;
        for (; r + 8 <= n_wide; r += 8) copy_rows<8, NT>(src, dst, plan, r, t, tid);
        if (r + 4 <= n_wide) { copy_rows<4, NT>(src, dst, plan, r, t, tid); r += 4; }
        if (r + 2 <= n_wide) { copy_rows<2, NT>(src, dst, plan, r, t, tid); r += 2; }
        if (r < n_wide) copy_rows<1, NT>(src, dst, plan, r, t, tid);
        for (r = n_wide; r < n_rows; ++r) {                  // 1- / 2-byte words: 1 or 2 KiB per tile, whole waves (wave-uniform predicate)
            const RowDesc rd = plan.row[r];
            const uint64_t pos = rd.col_off + wtile_off(t, rd.tile_stride, rd.word_bytes) + (uint64_t)tid * 16;
            if (tid * 16u < rd.bytes) *reinterpret_cast<uint4*>(dst + pos) = *reinterpret_cast<const uint4*>(src + pos);
        }
    } else {
        for (uint32_t r = 0; r < n_rows; ++r) {
            const RowDesc rd = plan.row[r];
            const uint64_t pos = wtile_off(t, rd.tile_stride, rd.word_bytes) + rd.roff + (uint64_t)tid * 16;
            const uint64_t slot0 = (uint64_t)t * TILE + (rd.roff + tid * 16u) / rd.word_bytes;   // first slot of this lane's 16 bytes
            if (slot0 < len && tid * 16u < rd.bytes)
                *reinterpret_cast<uint4*>(dst + rd.col_off + pos) = *reinterpret_cast<const uint4*>(src + rd.col_off + pos);
        }
    }
    // masks: 16 u64 words per tile per mask (copied whole, so stale bits beyond the source's
    // len are cleared in the destination)
    for (uint32_t i = tid; i < 16u * plan.n_masks; i += blockDim.x) {      // (16 components + the liveness mask = 272 words: more than one trip of 256 threads)
        const uint32_t m = i >> 4, wi = i & 15u;
        const uint64_t o = plan.mask_off[m] + ((uint64_t)t * 16 + wi) * 8;
        *reinterpret_cast<uint64_t*>(dst + o) = *reinterpret_cast<const uint64_t*>(src + o);
    }
    if (t == 0) {
        if (fin.enabled) __syncthreads();
        if (tid == 0) {
            if (fin.enabled) { hdr.checksum[0] = cks[0]; hdr.checksum[1] = 0; hdr.active = cks[1]; }
            *reinterpret_cast<Header*>(dst) = hdr;
        }
    }
}

// ------------------------------------------------------------------ k_particles_step
// The GgrsSchedule of examples/stress_tests/particles.rs:233-240 as one pass:
//   update_particles  (particles.rs:272-280)  v += g*dt ; x += v*dt     (unfused mul, add)
//   despawn_particles (particles.rs:282-289)  ttl -= 1 ; ttl == 0 -> despawn
// and, because translation and velocity are already in registers, the per-entity part of
// ComponentChecksumPlugin::update (component_checksum.rs:77-90) for the NEXT SaveWorld:
// per-workgroup XOR partials + live count, folded later by finalize_block.
// Algorithmic traffic: 64 B per live entity (12+12+8 read, same written).
//
// All 4 mask loads and all 8 column loads of a lane are issued unconditionally and together
// (slots up to the padded capacity are always mapped); per-entity conditions are selects, and
// only wave-uniform conditions guard the stores.
template <bool UPD, bool TTL, bool CKS_T, bool CKS_V>
__global__ __launch_bounds__(TPB) void k_particles_step(StepArgs a) {
    const uint32_t t = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t e0 = (uint64_t)t * TILE + (uint64_t)tid * 4;     // first of this lane's 4 slots
    const uint64_t tb4 = wtile_off(t, a.ts, 4) + (uint64_t)tid * 16;    // its 16 bytes inside a 4-byte column's tile row
    const uint64_t tb8 = wtile_off(t, a.ts, 8) + (uint64_t)tid * 32;    // its 32 bytes inside an 8-byte column's tile rows
    const uint64_t w0 = (uint64_t)t * 16 + wave * 4;                 // first mask word of this wave
    const uint32_t sh = (lane & 15u) * 4;
    const uint64_t wi = w0 + (lane >> 4);
    constexpr bool NEED_T = UPD || CKS_T, NEED_V = UPD || CKS_V;

    // ---- every load of the tile, back to back
    const uint64_t alive_w = *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + wi * 8);
    uint64_t pT_w = 0, pV_w = 0, pL_w = 0;
    if (NEED_T) pT_w = *reinterpret_cast<const uint64_t*>(a.state + a.off_pT + wi * 8);
    if (NEED_V) pV_w = *reinterpret_cast<const uint64_t*>(a.state + a.off_pV + wi * 8);
    if (TTL) pL_w = *reinterpret_cast<const uint64_t*>(a.state + a.off_pL + wi * 8);
    float4 tx[3], vv[3];
    ulonglong2 tl[2];
    if (NEED_T) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tx[k] = *reinterpret_cast<const float4*>(a.state + a.off_t[k] + tb4);
    }
    if (NEED_V) {
#pragma unroll
        for (int k = 0; k < 3; ++k) vv[k] = *reinterpret_cast<const float4*>(a.state + a.off_v[k] + tb4);
    }
    if (TTL) {
        tl[0] = *reinterpret_cast<const ulonglong2*>(a.state + a.off_ttl + tb8);
        tl[1] = *reinterpret_cast<const ulonglong2*>(a.state + a.off_ttl + tb8 + 16);
    }

    const uint32_t n_alive = (uint32_t)(alive_w >> sh) & 0xFu;
    const uint32_t n_T = (uint32_t)(pT_w >> sh) & 0xFu, n_V = (uint32_t)(pV_w >> sh) & 0xFu,
                   n_L = (uint32_t)(pL_w >> sh) & 0xFu;
    const uint32_t m_upd = UPD ? (n_alive & n_T & n_V) : 0u;   // Query<(&mut Transform,&mut Velocity)>
    const uint32_t m_ttl = TTL ? (n_alive & n_L) : 0u;         // Query<(Entity,&mut Ttl)>

    // ---- update_particles (selects, no per-lane branches)
    if (UPD) {
        const float dt = __uint_as_float(a.dt_bits);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gd = __fmul_rn(a.g[k], dt);           // gravity * time_step
            float* x = reinterpret_cast<float*>(&tx[k]);
            float* v = reinterpret_cast<float*>(&vv[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool on = (m_upd >> j) & 1u;
                const float nv = __fadd_rn(v[j], gd);                       // **velocity += ...
                const float nx = __fadd_rn(x[j], __fmul_rn(nv, dt));        // translation += **velocity * time_step
                v[j] = on ? nv : v[j];
                x[j] = on ? nx : x[j];
            }
        }
        if (__ballot(m_upd != 0) != 0) {                      // wave-uniform
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                *reinterpret_cast<float4*>(a.state + a.off_t[k] + tb4) = tx[k];
                *reinterpret_cast<float4*>(a.state + a.off_v[k] + tb4) = vv[k];
            }
        }
    }

    // ---- despawn_particles
    uint32_t kill = 0;
    if (TTL) {
        uint64_t* q = reinterpret_cast<uint64_t*>(&tl[0]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = (m_ttl >> j) & 1u;
            const uint64_t nq = q[j] - 1;                    // usize, wrapping
            q[j] = on ? nq : q[j];
            kill |= (on && nq == 0) ? (1u << j) : 0u;
        }
        if (__ballot(m_ttl != 0) != 0) {
            *reinterpret_cast<ulonglong2*>(a.state + a.off_ttl + tb8) = tl[0];
            *reinterpret_cast<ulonglong2*>(a.state + a.off_ttl + tb8 + 16) = tl[1];
        }
    }
    const uint32_t n_new = n_alive & ~kill;

    // ---- new liveness words for this wave's 256 slots: 4 ballots + scalar bit-interleave
    uint32_t cnt = 0;
    if (TTL) {
        const uint64_t b0 = __ballot((n_new >> 0) & 1u), b1 = __ballot((n_new >> 1) & 1u),
                       b2 = __ballot((n_new >> 2) & 1u), b3 = __ballot((n_new >> 3) & 1u);
        const bool any_kill = __ballot(kill != 0) != 0;
        uint64_t mine = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint64_t nw = spread4(b0 >> (16 * w)) | (spread4(b1 >> (16 * w)) << 1) |
                                (spread4(b2 >> (16 * w)) << 2) | (spread4(b3 >> (16 * w)) << 3);
            cnt += (uint32_t)__popcll(nw);
            if (lane == (uint32_t)w) mine = nw;
        }
        if (any_kill && lane < 4)
            *reinterpret_cast<uint64_t*>(a.state + a.off_alive + (w0 + lane) * 8) = mine;
    } else if (CKS_T || CKS_V) {
        cnt = (uint32_t)__popcll(__ballot(n_new & 1u)) + (uint32_t)__popcll(__ballot(n_new & 2u)) +
              (uint32_t)__popcll(__ballot(n_new & 4u)) + (uint32_t)__popcll(__ballot(n_new & 8u));
    }

    // ---- checksum partials of the post-step state
    if (CKS_T || CKS_V) {
        uint64_t hT = 0, hV = 0;
        const uint32_t c_T = CKS_T ? (n_new & n_T) : 0u, c_V = CKS_V ? (n_new & n_V) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t order = e0 + j;                   // RollbackOrdered::order == slot
            if (CKS_T) {
                const uint64_t h = sea_pair(order, sea_inner3(__float_as_uint(reinterpret_cast<float*>(&tx[0])[j]),
                                                              __float_as_uint(reinterpret_cast<float*>(&tx[1])[j]),
                                                              __float_as_uint(reinterpret_cast<float*>(&tx[2])[j])));
                hT ^= ((c_T >> j) & 1u) ? h : 0ULL;
            }
            if (CKS_V) {
                const uint64_t h = sea_pair(order, sea_inner3(__float_as_uint(reinterpret_cast<float*>(&vv[0])[j]),
                                                              __float_as_uint(reinterpret_cast<float*>(&vv[1])[j]),
                                                              __float_as_uint(reinterpret_cast<float*>(&vv[2])[j])));
                hV ^= ((c_V >> j) & 1u) ? h : 0ULL;
            }
        }
        __shared__ uint64_t sT[4], sV[4];
        __shared__ uint32_t sC[4];
        if (CKS_T) hT = wave_xor(hT);
        if (CKS_V) hV = wave_xor(hV);
        if (lane == 0) { sT[wave] = hT; sV[wave] = hV; sC[wave] = cnt; }
        __syncthreads();
        if (tid == 0) {
            if (CKS_T) a.part_T[t] = sT[0] ^ sT[1] ^ sT[2] ^ sT[3];
            if (CKS_V) a.part_V[t] = sV[0] ^ sV[1] ^ sV[2] ^ sV[3];
            a.part_cnt[t] = (uint64_t)sC[0] + sC[1] + sC[2] + sC[3];
        }
    }
}

// ------------------------------------------------------------------ fused request groups
// handle_requests (schedule_systems.rs:170-289) receives the WHOLE request list of a ggrs tick at once, and every request of a
// kernel-backed world is slot-local, so a run of requests  [Load?] (Save | Advance)*  executes as ONE pass: the kernel the library
// writes for the world at seal (kernel_gen.hpp, `ggrs_jit_tick`).  The hand-written kernels of rounds 1-3 (k_tick .. k_tick3) are gone:
// round 4 measured the generated kernel ahead of k_tick3 in every mode it still served (all 15 rows stored by every Save:
// 88.5 vs 115.5 us per launch at 1 M, profiles/r04a).  What is left here are the limits of a group's argument block.
constexpr int MAX_TICK_OPS = 40, MAX_TICK_SAVES = 16, MAX_TICK_STEPS = 24;

constexpr int FIN_TPB = 1024;
constexpr int GEN_MAX_CKS = MAX_COMPS;

// ------------------------------------------------------------------ k_checksum (generic)
// ComponentChecksumPlugin::update (component_checksum.rs:67-108) for any registered spec,
// plus the live count EntityChecksumPlugin needs (entity_checksum.rs:40).  grid = (tiles, n_cks)
// (n_cks == 0 still launches y = 1 for the count).  One slot per lane per step, so one ballot
// is exactly one mask word.
__global__ __launch_bounds__(TPB) void k_checksum(CksArgs a, const UnitDesc* __restrict__ units) {
    const uint32_t t = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t h = 0;
    uint32_t cnt = 0;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const uint64_t e = (uint64_t)t * TILE + (uint64_t)i * TPB + tid;
        const uint64_t wi = e >> 6;
        const uint64_t aw = *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + wi * 8);
        if (k == 0 && lane == 0) cnt += (uint32_t)__popcll(aw);
        if (a.n_cks == 0) continue;
        const uint64_t pw = *reinterpret_cast<const uint64_t*>(a.state + a.off_present[k] + wi * 8);
        if (((aw & pw) >> (e & 63)) & 1ULL) {
            SeaStream s;
            const uint32_t n = a.n_units[k], ub = a.unit_base[k];
#pragma unroll 1
            for (uint32_t u = 0; u < n; ++u) {
                const UnitDesc ud = units[ub + u];
                const uint8_t* p = a.state + col_at(ud.off, ud.ts, ud.wb, e);
                const uint64_t v = ud.wb == 4 ? (uint64_t)*reinterpret_cast<const uint32_t*>(p) : (ud.wb == 8 ? *reinterpret_cast<const uint64_t*>(p)
                                 : (ud.wb == 2 ? (uint64_t)*reinterpret_cast<const uint16_t*>(p) : (uint64_t)*p));
                s.write(v, ud.wb);
            }
            h ^= sea_pair(e, s.finish());
        }
    }
    __shared__ uint64_t sH[4];
    __shared__ uint32_t sC[4];
    h = wave_xor(h);
    if (lane == 0) { sH[wave] = h; sC[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        if (a.n_cks) a.parts[(uint64_t)k * a.part_stride + t] = sH[0] ^ sH[1] ^ sH[2] ^ sH[3];
        if (k == 0) a.part_cnt[t] = (uint64_t)sC[0] + sC[1] + sC[2] + sC[3];
    }
}

// ------------------------------------------------------------------ generic systems
// benches/bench.rs:30-46 (increment_foos ...), tests/component_rollback.rs:24-28
__global__ __launch_bounds__(TPB) void k_add_u32(uint8_t* state, uint64_t off_alive, uint64_t off_present,
                                                 uint64_t off_col, uint32_t ts, uint32_t delta, uint64_t len) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= len) return;
    const uint64_t m = *reinterpret_cast<const uint64_t*>(state + off_alive + (e >> 6) * 8) &
                       *reinterpret_cast<const uint64_t*>(state + off_present + (e >> 6) * 8);
    if ((m >> (e & 63)) & 1ULL) {
        uint32_t* p = reinterpret_cast<uint32_t*>(state + col_at(off_col, ts, 4, e));
        *p = *p + delta;
    }
}
// tests/synctest.rs:37-44 decrease_health: saturating_sub then despawn at 0.  One slot per
// lane: the wave's ballot IS the new 64-bit liveness word.  With `defer` the despawn is
// commands.entity(e).despawn_rollback() on an unconfirmed frame (despawn.rs:114-143): the entity is
// disabled -- RollbackDespawned(frame) -- instead of freed.
struct DespawnMarks { uint64_t off_disabled, off_dframe; };   // live-only side state (outside every snapshot)
__global__ __launch_bounds__(TPB) void k_sat_sub_despawn(uint8_t* state, uint64_t off_alive, uint64_t off_present,
                                                         uint64_t off_col, uint32_t ts, uint32_t amount, uint64_t len_pad64,
                                                         int defer, int32_t frame, DespawnMarks dm) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= len_pad64) return;                       // whole waves only (len padded to 64)
    const uint64_t aw = *reinterpret_cast<const uint64_t*>(state + off_alive + (e >> 6) * 8);
    const uint64_t pw = *reinterpret_cast<const uint64_t*>(state + off_present + (e >> 6) * 8);
    bool alive = (aw >> (e & 63)) & 1ULL;
    bool killed = false;
    if (alive && ((pw >> (e & 63)) & 1ULL)) {
        uint32_t* p = reinterpret_cast<uint32_t*>(state + col_at(off_col, ts, 4, e));
        const uint32_t v = *p >= amount ? *p - amount : 0u;
        *p = v;
        if (v == 0) { alive = false; killed = true; }
    }
    const uint64_t nw = __ballot(alive);
    if ((threadIdx.x & 63u) == 0 && nw != aw) *reinterpret_cast<uint64_t*>(state + off_alive + (e >> 6) * 8) = nw;
    if (defer) {
        const uint64_t kw = __ballot(killed);
        if (killed) *reinterpret_cast<int32_t*>(state + dm.off_dframe + e * 4) = frame;
        if ((threadIdx.x & 63u) == 0 && kw) *reinterpret_cast<uint64_t*>(state + dm.off_disabled + (e >> 6) * 8) |= kw;
    }
}

// ------------------------------------------------------------------ box_game (examples/box_game/box_game.rs)
// move_cube_system (box_game.rs:154-206), one slot per lane.  Query<(&mut Transform, &mut Velocity, &Player),
// With<Rollback>>: the entity needs all three components.  Every operation is a single correctly rounded IEEE
// op in the reference's order (Rust never contracts; the build uses -ffp-contract=off and HIP's default
// correctly rounded fp32 divide / sqrt); glam's Vec3::clamp_length_max is
//   len_sq = x*x + y*y + z*z;  if len_sq > max*max { max * (v / sqrt(len_sq)) } else { v }
// and f32::clamp is two compares.  friction_pow = FRICTION.powf(dt), computed by the host's libm.
struct BoxMoveArgs {
    uint8_t* state;
    uint64_t off_alive, off_pT, off_pV, off_pP;
    uint64_t off_t[3], off_v[3], off_handle;
    uint32_t ts_t, ts_v, ts_handle, pad0;   // tile strides of the three components' columns
    uint64_t len;
    uint32_t dt_bits, friction_pow_bits;
    float accel, max_speed, half_width;
    uint32_t n_inputs;
    uint8_t inputs[16];
};
__global__ __launch_bounds__(TPB) void k_box_move(BoxMoveArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= a.len) return;
    const uint64_t wi8 = (e >> 6) * 8, b = e & 63;
    const uint64_t m = *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + wi8) &
                       *reinterpret_cast<const uint64_t*>(a.state + a.off_pT + wi8) &
                       *reinterpret_cast<const uint64_t*>(a.state + a.off_pV + wi8) &
                       *reinterpret_cast<const uint64_t*>(a.state + a.off_pP + wi8);
    if (!((m >> b) & 1ULL)) return;
    const uint64_t handle = *reinterpret_cast<const uint64_t*>(a.state + col_at(a.off_handle, a.ts_handle, 8, e));
    if (handle >= a.n_inputs) return;                  // inputs[p.handle] would panic in the reference
    const uint8_t in = a.inputs[handle];
    const float dt = __uint_as_float(a.dt_bits), fp = __uint_as_float(a.friction_pow_bits);
    float* px = reinterpret_cast<float*>(a.state + col_at(a.off_t[0], a.ts_t, 4, e));
    float* pz = reinterpret_cast<float*>(a.state + col_at(a.off_t[2], a.ts_t, 4, e));
    float* py = reinterpret_cast<float*>(a.state + col_at(a.off_t[1], a.ts_t, 4, e));
    float* pvx = reinterpret_cast<float*>(a.state + col_at(a.off_v[0], a.ts_v, 4, e));
    float* pvy = reinterpret_cast<float*>(a.state + col_at(a.off_v[1], a.ts_v, 4, e));
    float* pvz = reinterpret_cast<float*>(a.state + col_at(a.off_v[2], a.ts_v, 4, e));
    float vx = *pvx, vy = *pvy, vz = *pvz, x = *px, y = *py, z = *pz;
    box_move_math(x, y, z, vx, vy, vz, in, dt, fp, a.accel, a.max_speed, a.half_width);
    *pvx = vx; *pvy = vy; *pvz = vz;
    *px = x; *py = y; *pz = z;
}

// ------------------------------------------------------------------ RollbackDespawned (snapshot/despawn.rs)
// Host-issued commands.entity(e).despawn_rollback() on an unconfirmed frame.
__global__ void k_mark_despawned(uint8_t* state, uint64_t off_alive, DespawnMarks dm, uint64_t slot, int32_t frame) {
    uint64_t* a = reinterpret_cast<uint64_t*>(state + off_alive + (slot >> 6) * 8);
    const uint64_t bitm = 1ULL << (slot & 63);
    if (!(*a & bitm)) return;
    *a &= ~bitm;
    *reinterpret_cast<uint64_t*>(state + dm.off_disabled + (slot >> 6) * 8) |= bitm;
    *reinterpret_cast<int32_t*>(state + dm.off_dframe + slot * 4) = frame;
}
// LoadWorldSystems::EntityResurrect (resurrect_entities, despawn.rs:69-87: markers > the loaded frame
// are removed) plus what EntitySnapshotPlugin::load's reconcile (entity.rs:55-99) means for
// NON-rollback components: an entity that survives the load (exists now AND is in the snapshot) or
// stays disabled keeps them; one that is freed, or re-created as a fresh Entity with the old
// RollbackId, does not have them any more.  Runs BEFORE the load's copy overwrites the live
// liveness mask (stream order).  One slot per lane: a wave's ballot is one mask word.
struct ReconcileArgs {
    uint8_t* live; const uint8_t* snap;
    uint64_t off_alive; DespawnMarks dm;
    uint32_t n_nr; int32_t frame;
    uint64_t n_slots_pad64;
    uint64_t nr_present_off[MAX_MASKS];
};
__global__ __launch_bounds__(TPB) void k_load_reconcile(ReconcileArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= a.n_slots_pad64) return;
    const uint64_t wi8 = (e >> 6) * 8;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t dis = *reinterpret_cast<const uint64_t*>(a.live + a.dm.off_disabled + wi8);
    const bool d = (dis >> lane) & 1ULL;
    const int32_t m = d ? *reinterpret_cast<const int32_t*>(a.live + a.dm.off_dframe + e * 4) : 0;
    const uint64_t res = __ballot(d && m > a.frame);              // despawned_frame > rollback_frame
    if (lane == 0) {
        const uint64_t alive_live = *reinterpret_cast<const uint64_t*>(a.live + a.off_alive + wi8);
        const uint64_t s_alive = *reinterpret_cast<const uint64_t*>(a.snap + a.off_alive + wi8);   // zero beyond the snapshot's len
        const uint64_t dis_after = dis & ~res;
        if (res) *reinterpret_cast<uint64_t*>(a.live + a.dm.off_disabled + wi8) = dis_after;
        const uint64_t keep = ((alive_live | res) & s_alive) | dis_after;
        for (uint32_t k = 0; k < a.n_nr; ++k) {
            uint64_t* p = reinterpret_cast<uint64_t*>(a.live + a.nr_present_off[k] + wi8);
            const uint64_t v = *p;
            if (v & ~keep) *p = v & keep;
        }
    }
}
// AdvanceWorldSystems::DespawnConfirmed (despawn_confirmed_entities, despawn.rs:89-112): disabled
// entities whose marked frame is <= ConfirmedFrameCount are freed for good.
__global__ __launch_bounds__(TPB) void k_despawn_confirmed(uint8_t* live, DespawnMarks dm, int32_t confirmed, uint64_t n_slots_pad64) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= n_slots_pad64) return;
    const uint64_t wi8 = (e >> 6) * 8;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t dis = *reinterpret_cast<const uint64_t*>(live + dm.off_disabled + wi8);
    const bool d = (dis >> lane) & 1ULL;
    const int32_t m = d ? *reinterpret_cast<const int32_t*>(live + dm.off_dframe + e * 4) : 0;
    const uint64_t gone = __ballot(d && m <= confirmed);
    if (lane == 0 && gone) *reinterpret_cast<uint64_t*>(live + dm.off_disabled + wi8) = dis & ~gone;
}
// BRANCH STEPS of worlds with live-only state (host_groups.hpp run_branch_step, host_fanout.hpp ggrs_hip_fanout_adopt).
// Adoption of a retained branch: its marker record -- per 64-slot unit the u64 of the slots the branch newly disabled, then (at frames_off) one i32 frame per
// such slot -- joins the live markers up to the adopted frame (markers are monotone inside a branch), and those entities stop being alive.  Queued BEFORE the
// adoption's LoadWorld: k_load_reconcile must find them disabled, so that they keep their non-rollback components.  One slot per lane; only the first n_units
// words of the record were written by the step's launch.
struct MaskOffs { uint64_t off[MAX_MASKS]; };
__global__ __launch_bounds__(TPB) void k_merge_branch_marks(uint8_t* live, uint64_t off_alive, DespawnMarks dm, const uint8_t* rec, uint64_t frames_off,
                                                            uint32_t n_units, int32_t frame) {
    const uint64_t e = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if ((e >> 6) >= n_units) return;                  // whole waves only
    const uint64_t wi8 = (e >> 6) * 8;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = *reinterpret_cast<const uint64_t*>(rec + wi8);
    const bool mine = (nw >> lane) & 1ULL;
    const int32_t m = mine ? *reinterpret_cast<const int32_t*>(rec + frames_off + e * 4) : 0;
    const bool take = mine && m <= frame;
    const uint64_t sel = __ballot(take);
    if (!sel) return;
    if (take) *reinterpret_cast<int32_t*>(live + dm.off_dframe + e * 4) = m;
    if (lane == 0) {
        *reinterpret_cast<uint64_t*>(live + dm.off_disabled + wi8) |= sel;
        *reinterpret_cast<uint64_t*>(live + off_alive + wi8) &= ~sel;
    }
}
// After a member launch: the entities some branch despawned for good (GgrsJitArgs::gone) lose their non-rollback components -- what the reconcile of the next
// LoadGameState does to them in the list form.  One mask word per thread.
__global__ __launch_bounds__(TPB) void k_clear_gone(uint8_t* live, const uint64_t* gone, uint32_t n_units, uint32_t n_nr, MaskOffs nr_present_off) {
    const uint32_t wi = blockIdx.x * TPB + threadIdx.x;
    if (wi >= n_units) return;
    const uint64_t g = gone[wi];
    if (!g) return;
    for (uint32_t k = 0; k < n_nr; ++k) {
        uint64_t* p = reinterpret_cast<uint64_t*>(live + nr_present_off.off[k] + (uint64_t)wi * 8);
        const uint64_t v = *p;
        if (v & g) *p = v & ~g;
    }
}

// THE PEER VIEW (ggrs_hip_add_custom_system_peers; host_world.hpp ggrs_world::PeerView).  Ahead of every request group that holds an AdvanceWorld, the peer-bound
// columns of the group's SOURCE block (tile-major) are copied into linear arrays, and the visibility words -- alive AND every peer-bound component present, cut at the
// source's len -- are built by plain word ANDs.  One 64-slot unit per wave: a lane moves one word per column (coalesced on both sides), lane 0 writes the unit's
// visibility word.  The tick launch that follows gathers from these arrays only: it may rewrite its source block in place.
constexpr int PEER_MAX_COLS = GGRS_PEER_MAX_COLUMNS;
struct PeerPubArgs {
    const uint8_t* src; uint64_t* vis; uint64_t len, off_alive;
    uint64_t off_present[PEER_MAX_COLS], col_off[PEER_MAX_COLS];
    uint8_t* dst[PEER_MAX_COLS];
    uint32_t ts[PEER_MAX_COLS], wb[PEER_MAX_COLS];
    uint32_t n_pres, n_cols, n_units;
};
__global__ __launch_bounds__(TPB) void k_publish_peers(PeerPubArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);             // this wave's 64-slot unit == its mask word
    if (u >= a.n_units) return;
    const uint64_t e = (uint64_t)u * 64u + lane;
    if (lane == 0) {
        uint64_t v = *reinterpret_cast<const uint64_t*>(a.src + a.off_alive + (uint64_t)u * 8u);
        for (uint32_t k = 0; k < a.n_pres; ++k) v &= *reinterpret_cast<const uint64_t*>(a.src + a.off_present[k] + (uint64_t)u * 8u);
        const uint64_t lo = (uint64_t)u * 64u;                                   // the source's len: slots at or beyond it are not entities of this frame
        v &= a.len >= lo + 64u ? ~0ull : (a.len > lo ? (1ull << (a.len - lo)) - 1ull : 0ull);
        a.vis[u] = v;
    }
    if (e >= a.len) return;
    for (uint32_t c = 0; c < a.n_cols; ++c) {
        const uint8_t* p = a.src + col_at(a.col_off[c], a.ts[c], a.wb[c], e);
        switch (a.wb[c]) {
        case 8: reinterpret_cast<uint64_t*>(a.dst[c])[e] = *reinterpret_cast<const uint64_t*>(p); break;
        case 4: reinterpret_cast<uint32_t*>(a.dst[c])[e] = *reinterpret_cast<const uint32_t*>(p); break;
        case 2: reinterpret_cast<uint16_t*>(a.dst[c])[e] = *reinterpret_cast<const uint16_t*>(p); break;
        default: a.dst[c][e] = *p; break;
        }
    }
}

// THE PEER INDEX (ggrs_hip_register_peer_index; host_world.hpp ggrs_world::PeerIndex).  Right behind every publish, the multimap key -> slots is rebuilt from the
// VIEW (the linear key column and the visibility words): a stable LSD radix sort of (key16, slot) pairs with 8-bit digits -- the input order is slot order, so
// stability alone gives ascending slots inside a bucket; a slot that is not indexed (not visible, or its key >= n_buckets) sorts as key 65535, behind every bucket.
// One pass when n_buckets <= 255, else two.  Per pass: k_ix_hist (a tile's digit histogram, into the digit-major table), k_ix_scan (one workgroup: the table's
// exclusive prefix sums), k_ix_scatter (the stable scatter).  Then k_ix_bounds writes ix_start from the sorted keys.  Nothing here depends on the order in which
// lanes, waves or workgroups arrive: the atomics only COUNT (integer adds commute), every position is counts + a rank built from ballots; and the work per slot does
// not depend on how the keys are distributed (a wave adds its digit count once per distinct digit: one bucket for everyone is the CHEAPEST case).  The kernel
// boundary is the only synchronisation.
constexpr uint32_t IX_TPB = 256, IX_ROUNDS = 8, IX_TILE = IX_TPB * IX_ROUNDS;      // a workgroup walks its 2048-slot tile in 8 rounds of 256, in slot order
constexpr uint32_t IX_NONE = 65535u, IX_SCAN_TPB = 1024;
struct IxArgs {
    const uint32_t* key_col; const uint64_t* vis;        // the first pass reads the view ...
    const uint32_t* key_in; const uint32_t* val_in;      // ... a later one the pairs the pass before it left
    uint32_t* key_out; uint32_t* val_out; uint32_t* hist;
    uint64_t n; uint32_t n_tiles, n_buckets, shift;
};
template <bool FIRST> __device__ __forceinline__ uint32_t ix_key(const IxArgs& a, uint64_t i) {
    if (!FIRST) return a.key_in[i];
    const uint32_t k = a.key_col[i];
    return ((a.vis[i >> 6] >> (i & 63ull)) & 1ull) && k < a.n_buckets ? k : IX_NONE;
}
// the lanes of the wave that hold the same digit as this one (a lane beyond the data matches nobody): one wave64 ballot per digit bit
__device__ __forceinline__ uint64_t ix_match(uint32_t d, bool act) {
    uint64_t m = __ballot(act);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) { const bool bit = (d >> b) & 1u; const uint64_t bal = __ballot(act && bit); m &= bit ? bal : ~bal; }
    return act ? m : 0ull;
}
// one tile's digit histogram into h (LDS, zeroed, a barrier behind the zeroing): 8 rounds; the caller puts a barrier behind it
template <bool FIRST> __device__ __forceinline__ void ix_hist_tile(const IxArgs& a, uint32_t tile, uint32_t* h) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    for (uint32_t r = 0; r < IX_ROUNDS; ++r) {
        const uint64_t i = (uint64_t)tile * IX_TILE + r * IX_TPB + t;
        const bool act = i < a.n;
        const uint32_t d = act ? (ix_key<FIRST>(a, i) >> a.shift) & 255u : 0u;
        const uint64_t m = ix_match(d, act);
        if (act && !(m & ((1ull << lane) - 1ull))) atomicAdd(&h[d], (uint32_t)__popcll(m));      // the lowest lane of every digit group adds the group's count
    }
}
template <bool FIRST> __global__ __launch_bounds__(IX_TPB) void k_ix_hist(IxArgs a) {
    __shared__ uint32_t h[256];
    const uint32_t t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    ix_hist_tile<FIRST>(a, blockIdx.x, h);
    __syncthreads();
    a.hist[(uint64_t)t * a.n_tiles + blockIdx.x] = h[t];
}
// exclusive prefix sums over the 256 x n_tiles table entries, in place, by ONE workgroup of 16 waves (as k_diff_scan: no look-back, nothing waits on another
// workgroup).  The table is n_tiles units of 256 words; a wave owns a contiguous run of units and walks it twice with 16-byte loads -- 64 lanes x 4 words, coalesced --:
// once for the run's total (the 16 totals meet in LDS), once to write the prefixes: a lane's four words, a shuffle scan across the wave, the wave's running carry
__global__ __launch_bounds__(IX_SCAN_TPB) void k_ix_scan(uint32_t* hist, uint32_t n_units) {
    __shared__ uint32_t tot[IX_SCAN_TPB / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t u0 = (uint32_t)((uint64_t)wv * n_units / (IX_SCAN_TPB / 64)), u1 = (uint32_t)((uint64_t)(wv + 1u) * n_units / (IX_SCAN_TPB / 64));
    uint4* const h4 = reinterpret_cast<uint4*>(hist);
    uint32_t s = 0;
    for (uint32_t u = u0; u < u1; ++u) { const uint4 v = h4[(uint64_t)u * 64u + lane]; s += v.x + v.y + v.z + v.w; }
    for (uint32_t off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) tot[wv] = s;
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t q = 0; q < wv; ++q) carry += tot[q];
    for (uint32_t u = u0; u < u1; ++u) {
        const uint4 v = h4[(uint64_t)u * 64u + lane];
        const uint32_t t = v.x + v.y + v.z + v.w;
        uint32_t inc = t;
        for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off); if (lane >= off) inc += o; }
        const uint32_t ex = carry + inc - t;
        h4[(uint64_t)u * 64u + lane] = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
        carry += __shfl(inc, 63);
    }
}
// one tile's stable scatter: base[d] (LDS) = where the tile's first pair of digit d goes, cnt (LDS) zeroed, a barrier behind both; ends on a barrier
template <bool FIRST> __device__ __forceinline__ void ix_scatter_tile(const IxArgs& a, uint32_t tile, uint32_t* base, uint32_t (*cnt)[256]) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    for (uint32_t r = 0; r < IX_ROUNDS; ++r) {
        const uint64_t i = (uint64_t)tile * IX_TILE + r * IX_TPB + t;
        const bool act = i < a.n;
        const uint32_t k = act ? ix_key<FIRST>(a, i) : 0u, d = (k >> a.shift) & 255u;
        const uint32_t v = FIRST ? (uint32_t)i : (act ? a.val_in[i] : 0u);
        const uint64_t m = ix_match(d, act), below = m & ((1ull << lane) - 1ull);
        if (act && !below) cnt[wv][d] = (uint32_t)__popcll(m);        // one plain store per distinct digit of the wave
        __syncthreads();
        if (act) {
            uint32_t pos = base[d] + (uint32_t)__popcll(below);         // the rank inside the wave: the lanes below with the same digit
            for (uint32_t q = 0; q < wv; ++q) pos += cnt[q][d];         // ... and the waves before it
            a.key_out[pos] = k; a.val_out[pos] = v;
        }
        __syncthreads();
        uint32_t add = 0;
        for (uint32_t q = 0; q < IX_TPB / 64; ++q) { add += cnt[q][t]; cnt[q][t] = 0; }
        base[t] += add;
        __syncthreads();
    }
}
template <bool FIRST> __global__ __launch_bounds__(IX_TPB) void k_ix_scatter(IxArgs a) {
    __shared__ uint32_t base[256], cnt[IX_TPB / 64][256];
    const uint32_t t = threadIdx.x;
    base[t] = a.hist[(uint64_t)t * a.n_tiles + blockIdx.x];            // where this tile's first pair of digit t goes
    for (uint32_t q = 0; q < IX_TPB / 64; ++q) cnt[q][t] = 0;
    __syncthreads();
    ix_scatter_tile<FIRST>(a, blockIdx.x, base, cnt);
}
// THE SMALL FORM: a world of at most IX_SMALL_TILES tiles (2048 slots) is sorted by ONE workgroup in ONE launch -- the same tile bodies, the tiles one after the
// other, the digit-major table and its scan in LDS, a barrier where the large form has a kernel boundary (the second pass reads pairs that other waves of this
// workgroup stored: a workgroup-scope fence and the barrier order them).  Such a world sits on the launch floor: 2 launches (this one, k_ix_bounds) instead of 4 or 7
constexpr uint32_t IX_SMALL_TILES = 1;      // measured (profiles/peer_index): one workgroup walks a tile in ~14 us per pass -- a win over 3 launches per pass for one tile, a loss from two tiles on
template <bool FIRST> __device__ __forceinline__ void ix_small_pass(const IxArgs& a, uint32_t* h, uint32_t* tab, uint32_t* base, uint32_t (*cnt)[256]) {
    const uint32_t t = threadIdx.x, T = a.n_tiles;
    for (uint32_t b = 0; b < T; ++b) {
        h[t] = 0;
        __syncthreads();
        ix_hist_tile<FIRST>(a, b, h);
        __syncthreads();
        tab[t * T + b] = h[t];
    }
    uint32_t sum = 0;                                                    // lane t owns digit t's T entries: the table is digit-major
    for (uint32_t b = 0; b < T; ++b) sum += tab[t * T + b];
    h[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < IX_TPB; off <<= 1) {
        const uint32_t v = t >= off ? h[t - off] : 0u;
        __syncthreads();
        h[t] += v;
        __syncthreads();
    }
    uint32_t run = h[t] - sum;
    for (uint32_t b = 0; b < T; ++b) { const uint32_t v = tab[t * T + b]; tab[t * T + b] = run; run += v; }
    for (uint32_t b = 0; b < T; ++b) {
        base[t] = tab[t * T + b];
        for (uint32_t q = 0; q < IX_TPB / 64; ++q) cnt[q][t] = 0;
        __syncthreads();
        ix_scatter_tile<FIRST>(a, b, base, cnt);
    }
    __threadfence_block();
    __syncthreads();
}
__global__ __launch_bounds__(IX_TPB) void k_ix_small(IxArgs a0, IxArgs a1, uint32_t passes) {
    __shared__ uint32_t h[256], tab[256 * IX_SMALL_TILES], base[256], cnt[IX_TPB / 64][256];
    ix_small_pass<true>(a0, h, tab, base, cnt);
    if (passes > 1) ix_small_pass<false>(a1, h, tab, base, cnt);
}
// ix_start[b], b = 0 .. n_buckets: the first position whose sorted key is >= b -- a binary search per bucket (n_buckets x log2 n loads whatever the keys are; empty
// buckets need no gap fill by a neighbour).  ix_start[n_buckets] is the number of indexed slots: every pair behind it carries IX_NONE
__global__ __launch_bounds__(IX_TPB) void k_ix_bounds(const uint32_t* keys, uint32_t* start, uint64_t n, uint32_t n_buckets) {
    const uint32_t b = blockIdx.x * IX_TPB + threadIdx.x;
    if (b > n_buckets) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (keys[mid] < b) lo = mid + 1; else hi = mid; }
    start[b] = (uint32_t)lo;
}

// THE INBOX (ggrs_hip_add_custom_system_effects; host_world.hpp ggrs_world::EffectInbox).  Right behind every request group that holds an AdvanceWorld, the sends the
// group's launch left in the inbox -- linear arrays, one word per slot and effect column, the op's identity where nothing was sent -- are combined into the LIVE block
// (tile-major) and the identities are put back.  One 64-slot unit per wave: a lane reads its inbox word (coalesced); a word that is not the identity is combined into
// the live column word when the slot is alive at the END of the frame and has the component, and dropped otherwise; either way the identity goes back.  Plain loads
// and stores: the sends were atomics of an EARLIER launch, and a slot is touched by one lane.
constexpr int FX_MAX_COLS = GGRS_EFFECT_MAX_COLUMNS;
struct FxApplyArgs {
    uint8_t* live; uint64_t len, off_alive;
    uint64_t off_present[FX_MAX_COLS], col_off[FX_MAX_COLS], ident[FX_MAX_COLS];
    uint8_t* inbox[FX_MAX_COLS];
    uint32_t ts[FX_MAX_COLS], wb[FX_MAX_COLS], op[FX_MAX_COLS];
    uint32_t n_cols, n_units;
};
// the identity of an effect op on a word of wb bytes (4 or 8): x op identity == x
__host__ __device__ inline uint64_t fx_identity(uint32_t op, uint32_t wb) {
    const uint64_t ones = wb == 8 ? ~0ull : 0xFFFFFFFFull;
    switch (op) {
    case GGRS_EFFECT_MIN_U: case GGRS_EFFECT_AND: return ones;
    case GGRS_EFFECT_MIN_I: return ones >> 1;                 // the largest signed value
    case GGRS_EFFECT_MAX_I: return (ones >> 1) + 1ull;        // the smallest
    default: return 0ull;                                     // ADD, MAX_U, OR, XOR
    }
}
template <typename U, typename I> __device__ __forceinline__ U fx_combine(uint32_t op, U x, U v) {
    switch (op) {
    case GGRS_EFFECT_ADD: return (U)(x + v);
    case GGRS_EFFECT_MIN_U: return v < x ? v : x;
    case GGRS_EFFECT_MAX_U: return v > x ? v : x;
    case GGRS_EFFECT_MIN_I: return (I)v < (I)x ? v : x;
    case GGRS_EFFECT_MAX_I: return (I)v > (I)x ? v : x;
    case GGRS_EFFECT_OR: return x | v;
    case GGRS_EFFECT_AND: return x & v;
    case GGRS_EFFECT_XOR: return x ^ v;
    default: return x;
    }
}
// one unit of k_apply_effects.  alive_known: the caller holds the unit's alive word in a register (k_apply_remote_effects: what its remote half just decided)
__device__ __forceinline__ void fx_apply_unit(const FxApplyArgs& a, uint32_t u, uint32_t lane, bool alive_known, uint64_t alive_w) {
    const uint64_t e = (uint64_t)u * 64u + lane;
    if (e >= a.len) return;                                                      // (a send never goes beyond the start-of-frame len, which the end-of-frame len is not below)
    for (uint32_t c = 0; c < a.n_cols; ++c) {
        if (a.wb[c] == 8) {
            uint64_t* in = reinterpret_cast<uint64_t*>(a.inbox[c]) + e;
            const uint64_t v = *in;
            if (v == a.ident[c]) continue;
            const uint64_t on = (alive_known ? alive_w : *reinterpret_cast<const uint64_t*>(a.live + a.off_alive + (uint64_t)u * 8u)) & *reinterpret_cast<const uint64_t*>(a.live + a.off_present[c] + (uint64_t)u * 8u);
            if ((on >> lane) & 1ull) { uint64_t* p = reinterpret_cast<uint64_t*>(a.live + col_at(a.col_off[c], a.ts[c], 8, e)); *p = fx_combine<uint64_t, int64_t>(a.op[c], *p, v); }
            *in = a.ident[c];
        } else {
            uint32_t* in = reinterpret_cast<uint32_t*>(a.inbox[c]) + e;
            const uint32_t v = *in;
            if (v == (uint32_t)a.ident[c]) continue;
            const uint64_t on = (alive_known ? alive_w : *reinterpret_cast<const uint64_t*>(a.live + a.off_alive + (uint64_t)u * 8u)) & *reinterpret_cast<const uint64_t*>(a.live + a.off_present[c] + (uint64_t)u * 8u);
            if ((on >> lane) & 1ull) { uint32_t* p = reinterpret_cast<uint32_t*>(a.live + col_at(a.col_off[c], a.ts[c], 4, e)); *p = fx_combine<uint32_t, int32_t>(a.op[c], *p, v); }
            *in = (uint32_t)a.ident[c];
        }
    }
}
__global__ __launch_bounds__(TPB) void k_apply_effects(FxApplyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);             // this wave's 64-slot unit == its mask word
    if (u >= a.n_units) return;
    fx_apply_unit(a, u, lane, false, 0ull);
}

// THE REMOTE INBOX (ggrs_hip_add_custom_system_remote; host_world.hpp ggrs_world::RemoteInbox).  Right behind every request group that holds an AdvanceWorld and AHEAD of
// k_apply_effects: the commands the group's launch ORed into the inbox -- one u32 per slot: bit 0 despawn, bits 1 + 2k / 2 + 2k insert / remove of remotely commanded
// component k -- are applied to the LIVE block.  One 64-slot unit per wave == one mask word; for slots below the end-of-frame len a lane reads its inbox word
// (coalesced).  A unit whose 64 words are all zero touches nothing else.  Otherwise the wave rebuilds the unit's alive word and each touched component's presence word
// with one __ballot each (lane 0 stores the 8-byte word), lanes whose slot gains a component write its registered default into the live columns (tile-major), and the
// inbox words go back to zero.  A command on a slot that is not alive once the frame's own despawns are in is dropped; DESPAWN WINS over everything, REMOVE WINS over
// insert.  Plain loads and stores: the sends were atomics of an EARLIER launch, a slot is touched by one lane, a mask word by one wave.
// VALUE BINDINGS (ggrs_hip_add_custom_system_values; ggrs_world::ValueInbox): bit 17 + k of the inbox word says a value was sent for component k.  The lane then reads
// the slot's winner word win[k][e] -- the largest key (g + 1) << 40 | (sender slot + 1) of the frame --, and where the slot gains the component it gathers the
// component's words from pay[g][..][sender] instead of the defaults: A VALUE WINS over a default insert, the winner's words arrive together.  The winner word goes back
// to zero whether the value landed or was dropped (a dead or despawned target, a remove); the payload needs no reset.
constexpr int RX_MAX_COMPS = GGRS_REMOTE_MAX_COMPONENTS;
constexpr int RX_MAX_WORDS = 64;                            // words of all remotely commanded components together (a world has at most 64 word columns)
struct RxApplyArgs {
    uint8_t* live; uint32_t* inbox; uint64_t len, off_alive;
    uint64_t off_present[RX_MAX_COMPS];
    uint64_t col_off[RX_MAX_WORDS], dflt[RX_MAX_WORDS];     // per word of component k, from w_base[k]: its column and the default it takes on insert
    uint32_t w_base[RX_MAX_COMPS], n_words[RX_MAX_COMPS], wb[RX_MAX_COMPS], ts[RX_MAX_COMPS];
    uint32_t n_comps, n_units;
    // value bindings: the winner words of component k (null: no value binding names it), the payload of the world's value binding g, the entries per payload word
    uint64_t* win[RX_MAX_COMPS]; const uint8_t* pay[GGRS_VALUE_MAX_WORLD_BINDINGS]; uint64_t pay_stride; uint32_t n_pay;
};
static_assert(sizeof(RxApplyArgs) + sizeof(FxApplyArgs) <= 4096, "RxApplyArgs travels by value beside FxApplyArgs (k_apply_remote_effects): both fit the 4 KiB kernel-argument segment");
// one unit of k_apply_remote, by all 64 lanes of its wave.  Returns whether the unit held a command; then alive_out is the unit's alive word as it stands now
__device__ __forceinline__ bool rx_apply_unit(const RxApplyArgs& a, uint32_t u, uint32_t lane, uint64_t& alive_out) {
    const uint64_t e = (uint64_t)u * 64u + lane;
    const bool inside = e < a.len;                                               // (a send never goes beyond the start-of-frame len, which the end-of-frame len is not below)
    const uint32_t m = inside ? a.inbox[e] : 0u;
    if (!__ballot(m != 0u)) return false;                                        // nothing was sent into this unit: nothing else is touched
    uint64_t* const alive_p = reinterpret_cast<uint64_t*>(a.live + a.off_alive + (uint64_t)u * 8u);
    const uint64_t alive_w = *alive_p;
    const bool alive = (alive_w >> lane) & 1ull;                                 // alive once the frame's own despawns are in: else every command is dropped
    const bool on = alive && !(m & 1u);                                          // despawn wins over everything
    const uint64_t alive_n = __ballot(on);
    alive_out = alive_n;
    if (lane == 0 && alive_n != alive_w) *alive_p = alive_n;
    for (uint32_t k = 0; k < a.n_comps; ++k) {
        const bool ins = (m >> (1u + 2u * k)) & 1u, rem = (m >> (2u + 2u * k)) & 1u;
        bool val = (m >> (17u + k)) & 1u;
        uint64_t key = 0;
        if (val) { key = a.win[k][e]; a.win[k][e] = 0ull; }                      // (the bit is only ever set beside a key, by the same sender)
        const uint32_t vg = (uint32_t)(key >> 40) - 1u;                          // the winner's value binding and slot
        const uint64_t vs = (key & 0xFFFFFFFFFFull) - 1ull;
        val = val && key != 0ull && vg < a.n_pay && vs < a.pay_stride;
        if (!__ballot(on && (ins || rem || val))) continue;                     // wave-uniform
        uint64_t* const pres_p = reinterpret_cast<uint64_t*>(a.live + a.off_present[k] + (uint64_t)u * 8u);
        const uint64_t pres_w = *pres_p;
        const bool has = (pres_w >> lane) & 1ull;
        const bool gains = on && (ins || val) && !rem;                           // remove wins over any insert
        const uint64_t pres_n = __ballot(on ? (!rem && (ins || val || has)) : has);
        if (lane == 0 && pres_n != pres_w) *pres_p = pres_n;
        if (gains && val) for (uint32_t q = 0; q < a.n_words[k]; ++q) {          // a value wins over a default insert: the winner's words, gathered from its payload slot
            uint8_t* const p = a.live + col_at(a.col_off[a.w_base[k] + q], a.ts[k], a.wb[k], e);
            // (vg differs per lane: a.pay[vg] is a vector load from the kernel-argument segment, not a copy of the block into scratch -- tests/test_remote_values_text.py
            // pins private_segment_fixed_size 0 for both apply kernels)
            const uint8_t* const v = a.pay[vg] + ((uint64_t)q * a.pay_stride + vs) * a.wb[k];
            if (a.wb[k] == 8) *reinterpret_cast<uint64_t*>(p) = *reinterpret_cast<const uint64_t*>(v);
            else *reinterpret_cast<uint32_t*>(p) = *reinterpret_cast<const uint32_t*>(v);
        }
        else if (gains) for (uint32_t q = 0; q < a.n_words[k]; ++q) {                 // Bevy's insert: a present component's value is replaced
            const uint32_t x = a.w_base[k] + q;
            uint8_t* const p = a.live + col_at(a.col_off[x], a.ts[k], a.wb[k], e);
            switch (a.wb[k]) {
            case 8: *reinterpret_cast<uint64_t*>(p) = a.dflt[x]; break;
            case 4: *reinterpret_cast<uint32_t*>(p) = (uint32_t)a.dflt[x]; break;
            case 2: *reinterpret_cast<uint16_t*>(p) = (uint16_t)a.dflt[x]; break;
            default: *p = (uint8_t)a.dflt[x]; break;
            }
        }
    }
    if (m) a.inbox[e] = 0u;
    return true;
}
__global__ __launch_bounds__(TPB) void k_apply_remote(RxApplyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);             // this wave's 64-slot unit == its mask word (wave-uniform)
    if (u >= a.n_units) return;
    uint64_t alive_w;
    (void)rx_apply_unit(a, u, lane, alive_w);
}
// A world with BOTH remote and effect bindings: k_apply_remote and k_apply_effects walk the same units of the same block, one wave per unit, and an effect looks at
// nothing of another unit -- so one launch does both, the remote half first.  The effects apply to the alive bits the remote commands left: where the unit held a
// command the wave carries its new alive word over in a register (lane 0's store of it is not read back), elsewhere the word in memory is unchanged.  The presence
// words and columns the remote half writes are never an effect column's (a component under both kinds of binding is refused at seal).
__global__ __launch_bounds__(TPB) void k_apply_remote_effects(RxApplyArgs r, FxApplyArgs f) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);             // (wave-uniform; both halves cover the units below the end-of-frame len)
    if (u >= r.n_units) return;
    uint64_t alive_w = 0;
    const bool known = rx_apply_unit(r, u, lane, alive_w);
    fx_apply_unit(f, u, lane, known, alive_w);
}

// THE REDUCE INBOX (ggrs_hip_add_custom_system_reduces; host_world.hpp ggrs_world::ReduceInbox).  Right behind every request group that holds an AdvanceWorld: ONE
// wave; lane s loads line s of the inbox (the op's identity beyond the last line), the lane pattern of wave_xor32 folds the lines per word -- `old` is the identity,
// so masked rows contribute nothing; a word moves as two halves and is combined as one op of its width --, one lane combines the result into the live block's current
// resource cell, and every lane puts the identities back.  Plain loads and stores: the waves' atomics belong to an EARLIER launch; the kernel boundary is the
// only synchronisation.
struct RdApplyArgs {
    uint8_t* inbox; uint8_t* cell;                          // cell: the live block's current resource cell, as the group's launch left it
    uint32_t stripes, n_words;
    uint32_t off[GGRS_RESOURCE_MAX_BYTES / 4], wb[GGRS_RESOURCE_MAX_BYTES / 4], op[GGRS_RESOURCE_MAX_BYTES / 4];
};
template <int CTRL, int ROWS> __device__ __forceinline__ uint64_t rd_fold_step(uint32_t op, uint32_t wb, uint64_t id, uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(id >> 32), (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xF, false);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)id, (int)(uint32_t)v, CTRL, ROWS, 0xF, false);
    return wb == 8 ? fx_combine<uint64_t, int64_t>(op, v, ((uint64_t)hi << 32) | lo) : (uint64_t)fx_combine<uint32_t, int32_t>(op, (uint32_t)v, lo);
}
__global__ __launch_bounds__(64) void k_apply_reduces(RdApplyArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = 0; k < a.n_words; ++k) {
        const uint32_t op = a.op[k], wb = a.wb[k];
        const uint64_t id = fx_identity(op, wb);
        uint64_t v = id;
        if (lane < a.stripes) {
            uint8_t* const p = a.inbox + (uint64_t)lane * 64u + a.off[k];
            if (wb == 8) { v = *reinterpret_cast<const uint64_t*>(p); *reinterpret_cast<uint64_t*>(p) = id; }
            else { v = *reinterpret_cast<const uint32_t*>(p); *reinterpret_cast<uint32_t*>(p) = (uint32_t)id; }
        }
        v = rd_fold_step<0xB1, 0xF>(op, wb, id, v);          // quad_perm:[1,0,3,2]
        v = rd_fold_step<0x4E, 0xF>(op, wb, id, v);          // quad_perm:[2,3,0,1]
        v = rd_fold_step<0x141, 0xF>(op, wb, id, v);         // row_half_mirror
        v = rd_fold_step<0x140, 0xF>(op, wb, id, v);         // row_mirror: every lane holds its row's value
        v = rd_fold_step<0x142, 0xA>(op, wb, id, v);         // row_bcast:15 into rows 1 and 3
        v = rd_fold_step<0x143, 0xC>(op, wb, id, v);         // row_bcast:31 into rows 2 and 3: lane 63 holds the total
        if (lane == 63u && v != id) {
            uint8_t* const c = a.cell + a.off[k];
            if (wb == 8) *reinterpret_cast<uint64_t*>(c) = fx_combine<uint64_t, int64_t>(op, *reinterpret_cast<const uint64_t*>(c), v);
            else *reinterpret_cast<uint32_t*>(c) = fx_combine<uint32_t, int32_t>(op, *reinterpret_cast<const uint32_t*>(c), (uint32_t)v);
        }
    }
}

// THE SUM PARTIALS (ggrs_hip_add_custom_system_sums; host_world.hpp ggrs_world::SumPartials).  Right behind every request group that holds an AdvanceWorld: ONE
// launch, one workgroup per summed word.  Entry u of the word's array is the balanced tree over the 64 slots of unit u, stored by that unit's wave in the launch
// that just ran; the units that launch covered are [0, n_units), everything beyond counts as -0.0 and is NEVER loaded (an entry there may be of an earlier, larger
// launch).  The workgroup continues the same tree -- pair 2i with 2i + 1, level by level: while more than SM_TPB values are left, a pass in which every thread folds
// aligned runs of 16 values (four levels in registers) from one buffer into the other, a workgroup barrier between passes; then the last ten levels in LDS, stride
// doubling in place (x[2s i] += x[2s i + s]: the operands are the two sibling sub-tree sums, and the add is commutative bit for bit).  -0.0 pads every level: the
// exact identity.  One lane then stores cell + T into the live block's current resource cell.  Plain loads and stores: the waves' stores belong to an EARLIER
// launch, the kernel boundary is the only synchronisation with it; within the workgroup a barrier orders a pass's stores ahead of the next pass's loads (one CU, one L1).
constexpr uint32_t SM_TPB = 1024, SM_FAN = 16;
struct SmApplyArgs {
    const uint8_t* part; uint8_t* tmp; uint8_t* cell;        // cell: the live block's current resource cell, as the group's launch (and k_apply_reduces) left it
    uint32_t n_units, units, tmp_entries, n_words;           // n_units: what the group's launch covered; units / tmp_entries: entries per word of the arrays
    uint32_t off[GGRS_SUM_MAX_WORDS], wb[GGRS_SUM_MAX_WORDS];
};
template <typename F> __device__ __forceinline__ F sm_neg_zero();
template <> __device__ __forceinline__ float sm_neg_zero<float>() { return __uint_as_float(0x80000000u); }
template <> __device__ __forceinline__ double sm_neg_zero<double>() { return __longlong_as_double((long long)0x8000000000000000ull); }
template <typename F> __device__ __forceinline__ void sm_fold_word(const SmApplyArgs& a, uint32_t k, F* lds) {
    const uint32_t t = threadIdx.x;
    const F nz = sm_neg_zero<F>();
    const uint8_t* src = a.part + (uint64_t)k * a.units * 8u;
    uint32_t n = a.n_units, pp = 0;
    while (n > SM_TPB) {
        const uint32_t m = (n + SM_FAN - 1u) / SM_FAN;
        uint8_t* const dst = a.tmp + ((uint64_t)k * 2u + pp) * a.tmp_entries * 8u;
        for (uint32_t c = t; c < m; c += SM_TPB) {
            F x[SM_FAN];
#pragma unroll
            for (uint32_t i = 0; i < SM_FAN; ++i) { const uint32_t at = c * SM_FAN + i; x[i] = at < n ? *reinterpret_cast<const F*>(src + (uint64_t)at * 8u) : nz; }
#pragma unroll
            for (uint32_t wd = SM_FAN; wd > 1u; wd >>= 1)
#pragma unroll
                for (uint32_t i = 0; i < wd / 2u; ++i) x[i] = x[2u * i] + x[2u * i + 1u];
            *reinterpret_cast<F*>(dst + (uint64_t)c * 8u) = x[0];
        }
        __syncthreads();
        src = dst; n = m; pp ^= 1u;
    }
    lds[t] = t < n ? *reinterpret_cast<const F*>(src + (uint64_t)t * 8u) : nz;
    __syncthreads();
    for (uint32_t st = 1; st < SM_TPB; st <<= 1) {
        if (t < SM_TPB / (2u * st)) lds[2u * st * t] = lds[2u * st * t] + lds[2u * st * t + st];
        __syncthreads();
    }
    if (t == 0) { F* const c = reinterpret_cast<F*>(a.cell + a.off[k]); *c = *c + lds[0]; }
}
__global__ __launch_bounds__(SM_TPB) void k_apply_sums(SmApplyArgs a) {
    __shared__ double s_lv[SM_TPB];
    const uint32_t k = blockIdx.x;
    if (k >= a.n_words) return;
    if (a.wb[k] == 8) sm_fold_word<double>(a, k, s_lv);
    else sm_fold_word<float>(a, k, reinterpret_cast<float*>(s_lv));
}

// System-scope release + acquire on whatever CU / XCD the wave lands on: `buffer_wbl2 sc0 sc1` writes the XCD's dirty L2 lines back,
// `buffer_inv sc0 sc1` drops its clean ones.  2048 single-wave workgroups cover all 8 XCDs (workgroup b lands on XCD b % 8).
__global__ void k_flush_l2() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, ""); }

// ------------------------------------------------------------------ spawn / mask edits
// Set liveness + presence bits for slots [first, first+count) (Rollback on_add hook,
// rollback.rs:45-59) and clear the live-only masks a fresh entity does not carry (non-rollback
// components outside its bundle, a stale RollbackDespawned marker).  One mask word per thread; each
// word is owned by exactly one thread.
__global__ __launch_bounds__(TPB) void k_set_mask_range(uint8_t* state, uint64_t first, uint64_t count,
                                                        uint32_t n_masks, MaskOffs mask_off_set,
                                                        uint32_t n_clear, MaskOffs mask_off_clear) {
    const uint64_t w_first = first >> 6, w_last = (first + count - 1) >> 6;
    const uint64_t wi = w_first + (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (wi > w_last) return;
    const uint64_t lo = wi * 64, hi = lo + 64;
    const uint64_t a = first > lo ? first : lo, b = (first + count) < hi ? (first + count) : hi;
    const uint32_t nb = (uint32_t)(b - a);
    const uint64_t bits = (nb == 64 ? ~0ULL : ((1ULL << nb) - 1ULL)) << (a - lo);
    for (uint32_t m = 0; m < n_masks; ++m) {
        uint64_t* p = reinterpret_cast<uint64_t*>(state + mask_off_set.off[m] + wi * 8);
        *p |= bits;
    }
    for (uint32_t m = 0; m < n_clear; ++m) {
        uint64_t* p = reinterpret_cast<uint64_t*>(state + mask_off_clear.off[m] + wi * 8);
        *p &= ~bits;
    }
}
__global__ void k_edit_mask_bit(uint8_t* state, uint64_t mask_off, uint64_t slot, int value) {
    uint64_t* p = reinterpret_cast<uint64_t*>(state + mask_off + (slot >> 6) * 8);
    if (value) *p |= 1ULL << (slot & 63); else *p &= ~(1ULL << (slot & 63));
}
// Fill one column over [first, first+count) with a constant word (component defaults).
__global__ __launch_bounds__(TPB) void k_fill_col(uint8_t* state, uint64_t col_off, uint32_t ts, uint32_t word_bytes,
                                                  uint64_t first, uint64_t count, uint64_t value) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= count) return;
    uint8_t* p = state + col_at(col_off, ts, word_bytes, first + i);
    if (word_bytes == 4) *reinterpret_cast<uint32_t*>(p) = (uint32_t)value;
    else if (word_bytes == 8) *reinterpret_cast<uint64_t*>(p) = value;
    else if (word_bytes == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)value;
    else *p = (uint8_t)value;
}
// spawn_particles (particles.rs:258-270) payload: Velocity(vx, vy, 0.0), Ttl(ttl); Transform gets
// its default through k_fill_col.  Also emits checksum partials for the new rows so a fused
// step's pending partials stay complete.
struct SpawnArgs {
    uint8_t* state;
    uint64_t off_t[3], off_v[3], off_ttl;
    uint32_t ts;                          // tile stride of the rollback word columns
    uint32_t t_default[3];
    const float* vx; const float* vy;
    uint64_t first, count, ttl;
    uint64_t* part_T; uint64_t* part_V; uint64_t* part_cnt;   // slots [0, gridDim.x)
    int cks_T, cks_V;
};
__global__ __launch_bounds__(TPB) void k_spawn_particles(SpawnArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * TPB + tid;
    uint64_t hT = 0, hV = 0;
    uint32_t cnt = 0;
    if (i < a.count) {
        const uint64_t e = a.first + i;
        const float vx = a.vx[i], vy = a.vy[i];
        *reinterpret_cast<float*>(a.state + col_at(a.off_v[0], a.ts, 4, e)) = vx;
        *reinterpret_cast<float*>(a.state + col_at(a.off_v[1], a.ts, 4, e)) = vy;
        *reinterpret_cast<float*>(a.state + col_at(a.off_v[2], a.ts, 4, e)) = 0.0f;
        *reinterpret_cast<uint64_t*>(a.state + col_at(a.off_ttl, a.ts, 8, e)) = a.ttl;
        if (a.cks_T) hT = sea_pair(e, sea_inner3(a.t_default[0], a.t_default[1], a.t_default[2]));
        if (a.cks_V) hV = sea_pair(e, sea_inner3(__float_as_uint(vx), __float_as_uint(vy), 0u));
        cnt = 1;
    }
    __shared__ uint64_t sT[4], sV[4];
    __shared__ uint32_t sC[4];
    hT = wave_xor(hT); hV = wave_xor(hV);
    cnt = (uint32_t)__popcll(__ballot(cnt));
    if (lane == 0) { sT[wave] = hT; sV[wave] = hV; sC[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        a.part_T[blockIdx.x] = sT[0] ^ sT[1] ^ sT[2] ^ sT[3];
        a.part_V[blockIdx.x] = sV[0] ^ sV[1] ^ sV[2] ^ sV[3];
        a.part_cnt[blockIdx.x] = (uint64_t)sC[0] + sC[1] + sC[2] + sC[3];
    }
}

// ------------------------------------------------------------------ k_gen_finalize
// Fold of k_tick_gen's per-wave partials: one 1024-thread workgroup per Save; any number of checksummed components.
struct GenFinArgs {
    const uint64_t* parts; uint32_t part_stride, n_parts, n_cks, n_saves;     // grid = n_saves x members (batch of identical groups)
    uint32_t n_rows;                                                          // rows per Save: n_cks + 1, and one more in a world with device resources (their checksum part, XORed in as it is)
    uint64_t save_len[MAX_TICK_SAVES];                                        // RollbackOrdered::len at each Save of the group (a fused spawn grows it)
    uint64_t* out;
    uint64_t* done; uint64_t seq;                                             // completion tag per workgroup in pinned host memory (nullptr: none), see read_back
    uint64_t* out2;                                                           // a second copy of every Checksum(u128) in DEVICE memory (nullptr: none): what the fan-out's all-gather sends from (host_fanout.hpp)
    const uint8_t* mtab; uint32_t mstride, moff_save_len;                     // batch members with records (kernel_gen.hpp): member m's save_len[k] = *(u64*)(mtab + m * mstride + moff_save_len + 8 k)
    const uint64_t* dev_save_len;                                             // spawns decided on the device: RollbackOrdered::len at Save k as the launch left it (nullptr: save_len above)
};
__global__ __launch_bounds__(FIN_TPB) void k_gen_finalize(GenFinArgs f) {
    // rows = the n_cks component XORs + the live count; the 16 waves split over the rows so that every row's loads are in
    // flight together (one latency round, not one per row)
    const uint32_t k = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr uint32_t NW = FIN_TPB / 64;
    __shared__ uint64_t acc[GEN_MAX_CKS + 2];
    const uint32_t nc = f.n_rows;
    if (tid < nc) acc[tid] = 0;
    __syncthreads();
    const uint32_t wpr = nc >= NW ? 1u : NW / nc;                     // waves per row
    for (uint32_t row = wave / wpr; row < nc; row += NW / wpr) {
        const uint64_t* p = f.parts + ((uint64_t)k * nc + row) * f.part_stride;
        const bool is_cnt = row == f.n_cks;
        uint64_t x = 0, sum = 0;
        // the rows sit in other XCDs' L2 / HBM: the fold is latency-bound unless every load of a lane is in flight at once --
        // 16 per trip (a 1 M-entity world: 3907 values per row over 5 waves = 13 per lane: ONE round trip)
        constexpr int INFL = 16;
        for (uint32_t i0 = (wave % wpr) * 64u + lane; i0 < f.n_parts; i0 += (uint32_t)INFL * wpr * 64u) {
            uint64_t v[INFL];
#pragma unroll
            for (int u = 0; u < INFL; ++u) { const uint32_t i = i0 + (uint32_t)u * wpr * 64u; v[u] = i < f.n_parts ? p[i] : 0ULL; }
#pragma unroll
            for (int u = 0; u < INFL; ++u) { x ^= v[u]; sum += v[u]; }
        }
        x = wave_xor(x);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) {
            if (is_cnt) atomicAdd(reinterpret_cast<unsigned long long*>(&acc[row]), (unsigned long long)sum);
            else atomicXor(reinterpret_cast<unsigned long long*>(&acc[row]), (unsigned long long)x);
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t total = 0;
        for (uint32_t c = 0; c < f.n_cks; ++c) total ^= sea_one(acc[c]);      // component_checksum.rs:92-95
        const uint64_t len_k = f.dev_save_len ? f.dev_save_len[k % f.n_saves] : f.mtab ? *reinterpret_cast<const uint64_t*>(f.mtab + (uint64_t)(k / f.n_saves) * f.mstride + f.moff_save_len + 8u * (k % f.n_saves)) : f.save_len[k % f.n_saves];
        total ^= sea_pair(acc[f.n_cks], len_k);                               // entity_checksum.rs:29-52; XOR fold checksum.rs:88-99
        if (nc > f.n_cks + 1u) total ^= acc[f.n_cks + 1u];                    // resource_checksum.rs:63-83: the resources' part(s), hashed by the launch
        f.out[2 * (uint64_t)k] = total; f.out[2 * (uint64_t)k + 1] = 0;
        if (f.out2) { f.out2[2 * (uint64_t)k] = total; f.out2[2 * (uint64_t)k + 1] = 0; }
        // the result first, then the tag the waiting host polls (both in the same pinned allocation; release at system scope orders them)
        if (f.done) __hip_atomic_store(f.done + k, f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------ k_ff_fold
// Fold-forward without a following request-group launch (ff_flush): one 256-thread workgroup per chunk of a partial row of the LAST launch
// (device_prelude.hpp ff_fold_row) -- {value, tag} as one 16-byte cell into pinned host memory.  Workgroup b = row b / split, chunk b % split.
struct FfArgs { const uint64_t* rows; uint64_t* out; uint64_t seq; uint32_t nvals, g, stride, istride, nc1, split, cnt_row; };
__global__ __launch_bounds__(TPB) void k_ff_fold(FfArgs f) {
    const uint32_t b = blockIdx.x;
    if (b >= f.nvals * f.split) return;
    const uint32_t row = b / f.split, ck = b % f.split, per = (f.g + f.split - 1u) / f.split;
    ff_fold_row(f.rows + (uint64_t)row * f.stride, f.istride, ck * per, min(f.g, (ck + 1u) * per), (row % f.nc1) == f.cnt_row, f.out + 2u * b, f.seq);
}

// ------------------------------------------------------------------ STATE DIFF (ggrs_hip_diff_frames / ggrs_hip_diff_block)
// Where do two packed state blocks differ, under the world's own rules: a slot at or beyond a side's len is dead there, a slot dead on both sides holds no state, a
// component absent on both sides holds no state, where the alive bits differ only that is said, words are compared as bits.  Three launches, ordered by their
// boundaries alone (no compare-and-swap, no wait between workgroups):
//   k_diff_count   one 64-slot unit per wave-iteration, one slot per lane.  The unit's alive word and presence words of both sides are wave-uniform loads; every
//                  compared column is one coalesced tile-major load per side (col_at, the 8192-slot layout tiles), the inequality a __ballot masked by
//                  "alive and present on both sides".  Per-component counts are popcounts of those ballots, summed per workgroup in LDS, one 64-bit atomic add
//                  per non-zero counter and workgroup into the report (integer adds: order-free).  One u64 "any difference" ballot per unit is stored.
//   k_diff_scan    one workgroup: the exclusive prefix sum of the units' popcounts = every unit's first entry.
//   k_diff_emit    the non-zero units whose first entry is below max_entries are read again; a differing lane writes its entry at offset + (differing lanes
//                  below it).  Units are in slot order and so are the lanes of one: the entries are the lowest differing slots, ascending, whatever the grid is.
constexpr int DIFF_MAX_COLS = 64;                          // column_diff is one u64
constexpr uint32_t DIFF_BATCH = 4;                         // columns of one component whose loads are issued together
constexpr uint32_t DIFF_CNT_ENT = 0, DIFF_CNT_ALIVE = 1, DIFF_CNT_PRES = 2, DIFF_CNT_VAL = 2 + 64, DIFF_CNT_RES = 2 + 128, DIFF_CNT_WORDS = 2 + 128 + 1;
struct DiffArgs {
    const uint8_t* a; const uint8_t* b;
    uint64_t len_a, len_b, off_alive;
    uint64_t off_present[MAX_COMPS];                       // per COMPARED component j (rollback components, in id order)
    uint64_t col_off[DIFF_MAX_COLS];                       // per compared column q (grouped by component, ascending column number)
    uint64_t* unit_any; uint64_t* unit_off; uint64_t* cnt; ggrs_diff_entry* entries;
    uint32_t ts, n_comps, n_units, max_entries;
    uint32_t res_off_a, res_off_b, n_res;                  // the current resource cell of each side (byte offset inside the block)
    uint16_t res_lanes[GGRS_RESOURCE_MAX];                 // bit i: the i-th u32 of a cell belongs to resource r
    uint8_t comp_id[MAX_COMPS], comp_col0[MAX_COMPS], comp_ncols[MAX_COMPS];   // the world's component index; its first compared column q and how many
    uint8_t col_wb[DIFF_MAX_COLS], col_k[DIFF_MAX_COLS], col_word[DIFF_MAX_COLS];   // word bytes; the world's column number (the bit of column_diff); the word inside its component
};
__device__ __forceinline__ uint64_t diff_len_mask(uint64_t len, uint64_t lo) { return len >= lo + 64u ? ~0ull : (len > lo ? (1ull << (len - lo)) - 1ull : 0ull); }
__device__ __forceinline__ uint64_t diff_load(const uint8_t* p, uint32_t wb) {
    switch (wb) {
    case 8: return *reinterpret_cast<const uint64_t*>(p);
    case 4: return *reinterpret_cast<const uint32_t*>(p);
    case 2: return *reinterpret_cast<const uint16_t*>(p);
    default: return *p;
    }
}
struct DiffLane { uint64_t pres = 0, cols = 0, first_a = 0, first_b = 0; uint32_t first_comp = 0xFFFFFFFFu, first_word = 0xFFFFFFFFu; };
// one unit.  Returns the unit's "any difference" ballot and its alive-differs ballot; EMIT: also this lane's entry fields; else the per-component counts go to s_cnt (LDS)
template <bool EMIT> __device__ __forceinline__ uint64_t diff_unit(const DiffArgs& a, uint32_t u, uint32_t lane, unsigned long long* s_cnt, uint64_t* alive_x, uint64_t* alive_a, DiffLane* dl) {
    const uint64_t lo = (uint64_t)u * 64u, e = lo + lane;
    const uint64_t aa = *reinterpret_cast<const uint64_t*>(a.a + a.off_alive + (uint64_t)u * 8u) & diff_len_mask(a.len_a, lo);
    const uint64_t ab = *reinterpret_cast<const uint64_t*>(a.b + a.off_alive + (uint64_t)u * 8u) & diff_len_mask(a.len_b, lo);
    const uint64_t both = aa & ab;
    uint64_t any = aa ^ ab;
    *alive_x = any; *alive_a = aa;
    for (uint32_t j = 0; j < a.n_comps; ++j) {
        const uint64_t pa = *reinterpret_cast<const uint64_t*>(a.a + a.off_present[j] + (uint64_t)u * 8u);
        const uint64_t pb = *reinterpret_cast<const uint64_t*>(a.b + a.off_present[j] + (uint64_t)u * 8u);
        const uint64_t pd = (pa ^ pb) & both, common = pa & pb & both;
        uint64_t vd = 0;
        if (common) {                                                            // (wave-uniform: nobody has the component on both sides -> its columns are not read)
            const uint32_t q1 = (uint32_t)a.comp_col0[j] + a.comp_ncols[j];
            for (uint32_t q0 = a.comp_col0[j]; q0 < q1; q0 += DIFF_BATCH) {      // DIFF_BATCH columns' loads of both sides in flight before the first compare
                uint64_t va[DIFF_BATCH], vb[DIFF_BATCH];
#pragma unroll
                for (uint32_t i = 0; i < DIFF_BATCH; ++i) {
                    va[i] = 0; vb[i] = 0;
                    if (q0 + i < q1) {                                           // (wave-uniform)
                        const uint32_t wb = a.col_wb[q0 + i];
                        const uint64_t off = col_at(a.col_off[q0 + i], a.ts, wb, e);   // e < the padded capacity: inside the column for every lane
                        va[i] = diff_load(a.a + off, wb); vb[i] = diff_load(a.b + off, wb);
                    }
                }
#pragma unroll
                for (uint32_t i = 0; i < DIFF_BATCH; ++i) {
                    const uint64_t ne = __ballot(va[i] != vb[i]) & common;       // (a column beyond the component's last: 0 != 0 for nobody)
                    vd |= ne;
                    if (EMIT && ((ne >> lane) & 1ull)) {
                        if (!dl->cols) { dl->first_comp = a.comp_id[j]; dl->first_word = a.col_word[q0 + i]; dl->first_a = va[i]; dl->first_b = vb[i]; }
                        dl->cols |= 1ull << a.col_k[q0 + i];
                    }
                }
            }
        }
        if (EMIT) { if ((pd >> lane) & 1ull) dl->pres |= 1ull << a.comp_id[j]; }
        else if (lane == 0) {
            if (pd) atomicAdd(&s_cnt[DIFF_CNT_PRES + a.comp_id[j]], (unsigned long long)__popcll(pd));
            if (vd) atomicAdd(&s_cnt[DIFF_CNT_VAL + a.comp_id[j]], (unsigned long long)__popcll(vd));
        }
        any |= pd | vd;
    }
    return any;
}
__global__ __launch_bounds__(TPB) void k_diff_count(DiffArgs a) {
    __shared__ unsigned long long s_cnt[DIFF_CNT_RES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (uint32_t i = tid; i < DIFF_CNT_RES; i += TPB) s_cnt[i] = 0;
    __syncthreads();
    for (uint32_t u = blockIdx.x * (TPB / 64) + wave; u < a.n_units; u += gridDim.x * (TPB / 64)) {
        uint64_t ax, aa;
        const uint64_t any = diff_unit<false>(a, u, lane, s_cnt, &ax, &aa, nullptr);
        if (lane == 0) {
            a.unit_any[u] = any;
            if (any) atomicAdd(&s_cnt[DIFF_CNT_ENT], (unsigned long long)__popcll(any));
            if (ax) atomicAdd(&s_cnt[DIFF_CNT_ALIVE], (unsigned long long)__popcll(ax));
        }
    }
    // device resources: the current cell of each side, u32 by u32 (one wave of the launch; the word is zero before it and nobody else writes it)
    if (blockIdx.x == 0 && wave == 0 && a.n_res) {
        const uint32_t ra = lane < GGRS_RESOURCE_MAX_BYTES / 4 ? reinterpret_cast<const uint32_t*>(a.a + a.res_off_a)[lane] : 0u;
        const uint32_t rb = lane < GGRS_RESOURCE_MAX_BYTES / 4 ? reinterpret_cast<const uint32_t*>(a.b + a.res_off_b)[lane] : 0u;
        const uint64_t ne = __ballot(ra != rb);
        if (lane == 0) {
            uint64_t m = 0;
            for (uint32_t r = 0; r < a.n_res; ++r) if (ne & a.res_lanes[r]) m |= 1ull << r;
            a.cnt[DIFF_CNT_RES] = m;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < DIFF_CNT_RES; i += TPB) { const unsigned long long v = s_cnt[i]; if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.cnt) + i, v); }
}
__global__ __launch_bounds__(TPB) void k_diff_scan(const uint64_t* __restrict__ unit_any, uint64_t* __restrict__ unit_off, uint32_t n_units) {
    __shared__ uint64_t s[TPB];
    const uint32_t tid = threadIdx.x, per = (n_units + TPB - 1u) / TPB;
    const uint32_t lo = min(n_units, tid * per), hi = min(n_units, lo + per);
    uint64_t sum = 0;
#pragma unroll 8
    for (uint32_t i = lo; i < hi; ++i) sum += (uint64_t)__popcll(unit_any[i]);      // (a lane's words are consecutive: its loads are independent, eight in flight)
    s[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < TPB; o <<= 1) {
        const uint64_t v = tid >= o ? s[tid - o] : 0ull;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    uint64_t run = s[tid] - sum;
#pragma unroll 8
    for (uint32_t i = lo; i < hi; ++i) { unit_off[i] = run; run += (uint64_t)__popcll(unit_any[i]); }
}
__global__ __launch_bounds__(TPB) void k_diff_emit(DiffArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (uint32_t u = blockIdx.x * (TPB / 64) + wave; u < a.n_units; u += gridDim.x * (TPB / 64)) {
        const uint64_t any = a.unit_any[u], off = a.unit_off[u];
        if (!any || off >= a.max_entries) continue;                              // (wave-uniform)
        DiffLane dl; uint64_t ax, aa;
        (void)diff_unit<true>(a, u, lane, nullptr, &ax, &aa, &dl);
        const uint64_t idx = off + (uint64_t)__popcll(any & ((1ull << lane) - 1ull));
        if (((any >> lane) & 1ull) && idx < a.max_entries) {                     // (the lanes meet again before the next unit's ballots)
            ggrs_diff_entry* o = a.entries + idx;
            const uint32_t xa = (uint32_t)((aa >> lane) & 1ull);
            o->slot = (uint64_t)u * 64u + lane;
            o->alive_a = xa; o->alive_b = xa ^ (uint32_t)((ax >> lane) & 1ull);
            o->presence_diff = dl.pres; o->column_diff = dl.cols;
            o->first_comp = dl.first_comp; o->first_word = dl.first_word;
            o->first_a = dl.first_a; o->first_b = dl.first_b;
        }
    }
}

// ------------------------------------------------------------------ CHECKSUM PARTS (ggrs_hip_checksum_parts / ggrs_hip_checksum_parts_block)
// The per-component ChecksumParts of ONE complete packed block (component_checksum.rs:67-108, entity_checksum.rs:29-52, resource_checksum.rs:63-83), the values the
// tick folds into Checksum(u128) inside its launch and keeps none of.  A read-only pass of two launches, ordered by their boundary alone:
//   k_parts_hash    one 64-slot unit per wave-iteration, one slot per lane, grid-stride over the units of [0, len).  The unit's alive word (cut by len) and every
//                   spec's presence word are wave-uniform loads; a spec nobody of the unit holds reads no column.  Otherwise a lane that is alive and has the
//                   component feeds its registered words (col_at: tile-major, 1, 2, 4 or 8 bytes each) to a SeaStream and pairs the result with its slot
//                   (RollbackOrdered::order == slot); wave_xor makes the unit's value.  Accumulator rows per wave in LDS, one atomic per non-zero cell and workgroup
//                   into one of PARTS_STRIPES copies of the row (parts_shared.hpp, shared with the kernel generated for worlds with a user-written hasher).
//   k_parts_finish  one workgroup: the copies folded, sea_one per component, sea_pair(active, len), the resources' SeaStreams over the block's current cell, the XOR of all parts.
#define GGRS_SHARED_CODE(...) __VA_ARGS__
#include "parts_shared.hpp"
#undef GGRS_SHARED_CODE
static_assert(PARTS_MAX == MAX_COMPS && PARTS_WAVES * 64 == TPB, "parts_shared.hpp spells the limits of this file");
static_assert(sizeof(PartsWord) == sizeof(UnitDesc) && offsetof(PartsWord, wb) == offsetof(UnitDesc, wb) && offsetof(PartsWord, ts) == offsetof(UnitDesc, ts), "k_parts_hash reads the world's UnitDesc table");
constexpr uint32_t PARTS_ACC_BYTES = PARTS_STRIPES * PARTS_STRIPE_CELLS * 8;   // the scratch: the copies of the accumulator row ...
constexpr uint32_t PARTS_OUT_OFF = 20480;                  // ... then (here) the report followed by the parts
constexpr uint32_t PARTS_OUT_PARTS = 64;                   // ... the parts start this far behind the report
constexpr uint32_t PARTS_OUT_BYTES = 4096;
constexpr uint32_t PARTS_SCRATCH_BYTES = PARTS_OUT_OFF + PARTS_OUT_BYTES;
constexpr uint32_t PARTS_MAX_PARTS = MAX_COMPS + 1 + GGRS_RESOURCE_MAX;
static_assert(PARTS_CELLS <= PARTS_STRIPE_CELLS && PARTS_STRIPE_CELLS % 8 == 0 && PARTS_ACC_BYTES <= PARTS_OUT_OFF && PARTS_OUT_PARTS + PARTS_MAX_PARTS * sizeof(ggrs_checksum_part) <= PARTS_OUT_BYTES && sizeof(ggrs_parts_report) <= PARTS_OUT_PARTS, "the scratch holds every world's parts");
struct PartsFinArgs {
    const unsigned long long* acc; const uint8_t* res_cell; uint8_t* out;
    uint64_t len;
    uint32_t n_cks, n_res;
    uint32_t comp_id[MAX_COMPS];
    uint32_t res_id[GGRS_RESOURCE_MAX];
    uint8_t res_wb[GGRS_RESOURCE_MAX], res_nw[GGRS_RESOURCE_MAX], res_off[GGRS_RESOURCE_MAX][MAX_UNITS];   // per checksummed resource: word bytes, chosen words, each one's byte offset inside a cell
};
__global__ __launch_bounds__(TPB) void k_parts_hash(PartsArgs a) {
    __shared__ unsigned long long s_rows[PARTS_WAVES * PARTS_CELLS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    parts_rows_clear(s_rows);
    unsigned long long* const row = s_rows + wave * PARTS_CELLS;
    for (uint32_t u = blockIdx.x * PARTS_WAVES + wave; u < a.n_units; u += gridDim.x * PARTS_WAVES) {
        const uint64_t alive = parts_alive(a, u);
        if (!alive) continue;                                                    // (wave-uniform)
        const uint64_t e = (uint64_t)u * 64u + lane;
        if (lane == 0u) row[2u * a.n_cks] += (unsigned long long)__popcll(alive);
        for (uint32_t k = 0; k < a.n_cks; ++k) {
            const uint64_t m = alive & parts_present(a, k, u);
            if (!m) continue;                                                    // (wave-uniform: nobody of the unit holds the component -> no column is read)
            uint64_t h = 0;
            if ((m >> lane) & 1ull) {                                            // (a hashed lane is alive: its slot is below len, inside every column)
                SeaStream s;
                const uint32_t w0 = a.word_base[k], w1 = w0 + a.n_words[k];
#pragma unroll 1
                for (uint32_t i = w0; i < w1; ++i) {
                    const PartsWord pw = a.words[i];
                    s.write(parts_load(a.state + parts_col_at(pw.off, pw.ts, pw.wb, e), pw.wb), pw.wb);
                }
                h = sea_pair(e, s.finish());
            }
            parts_put(row, a.n_cks, k, h, m, lane);
        }
    }
    parts_rows_flush(a, s_rows);
}
__global__ __launch_bounds__(TPB) void k_parts_finish(PartsFinArgs f) {
    __shared__ uint64_t s_val[PARTS_MAX_PARTS];
    __shared__ uint64_t s_cell[PARTS_CELLS];
    const uint32_t t = threadIdx.x, n_parts = f.n_cks + 1u + f.n_res;
    ggrs_checksum_part* const parts = reinterpret_cast<ggrs_checksum_part*>(f.out + PARTS_OUT_PARTS);
    if (t <= 2u * f.n_cks) {                                                     // the copies of the row folded: XOR for the hashes, the sum for the counts
        uint64_t v = 0;
        for (uint32_t s = 0; s < (uint32_t)PARTS_STRIPES; ++s) { const uint64_t c = f.acc[s * (uint32_t)PARTS_STRIPE_CELLS + t]; v = t < f.n_cks ? v ^ c : v + c; }
        s_cell[t] = v;
    }
    __syncthreads();
    const uint64_t active = s_cell[2u * f.n_cks];
    if (t < n_parts) {
        ggrs_checksum_part p;
        if (t < f.n_cks) { p.kind = GGRS_PART_COMPONENT; p.id = f.comp_id[t]; p.value = sea_one(s_cell[t]); p.n_hashed = s_cell[f.n_cks + t]; }      // component_checksum.rs:92-95: nobody holds it -> sea_one(0)
        else if (t == f.n_cks) { p.kind = GGRS_PART_ENTITY; p.id = 0; p.value = sea_pair(active, f.len); p.n_hashed = active; }                       // entity_checksum.rs:29-52
        else {
            const uint32_t r = t - f.n_cks - 1u, wb = f.res_wb[r];
            SeaStream s;
            for (uint32_t i = 0; i < f.res_nw[r]; ++i) s.write(parts_load(f.res_cell + f.res_off[r][i], wb), wb);
            p.kind = GGRS_PART_RESOURCE; p.id = f.res_id[r]; p.value = s.finish(); p.n_hashed = 0;
        }
        parts[t] = p;
        s_val[t] = p.value;
    }
    __syncthreads();
    if (t == 0) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < n_parts; ++i) total ^= s_val[i];                // checksum.rs:88-99
        ggrs_parts_report rep;
        rep.len = f.len; rep.active = active; rep.checksum_lo = total; rep.checksum_hi = 0; rep.n_parts = n_parts;
        *reinterpret_cast<ggrs_parts_report*>(f.out) = rep;
    }
}

// ------------------------------------------------------------------ QUERY (ggrs_hip_query / ggrs_hip_query_block)
// Query<(&A, &B), (With<C>, Without<D>)> over one packed block: the live entities below len that have every With component and no Without component, gathered
// into dense output columns in ascending slot order.  The same stream compaction as the state diff with another predicate and a wide payload; three launches,
// ordered by their boundaries alone (no compare-and-swap, no wait between workgroups):
//   k_query_match  one 64-slot unit per LANE: the predicate needs only mask words (alive, one presence word per filtered component), and consecutive units' words
//                  are consecutive, so every mask is one coalesced load.  The unit's match word is stored; the word behind the last unit is a zero sentinel.
//   k_diff_scan    as it is, over n_units + 1 words: every unit's first row, and behind the last unit the number of matches.
//   k_query_emit   one unit per wave-iteration; units without a match and units whose first row is at or beyond max_rows are skipped.  A matching lane loads its
//                  fetched words (col_at, 1 / 2 / 4 / 8 bytes), QUERY_BATCH columns' loads before the first store, and stores them at row offset + (matching
//                  lanes below it): a unit's rows are contiguous in every output column.  Nothing at or beyond row max_rows is written.
constexpr uint32_t QUERY_BATCH = 4;                        // fetched columns whose loads are issued together
struct QueryArgs {
    const uint8_t* state; uint8_t* out;
    uint64_t len, max_rows, off_alive, slots_off;
    uint64_t off_mask[MAX_COMPS];                          // presence masks of the filtered components (With first or not: bit j of without says which)
    uint64_t col_off[GGRS_QUERY_MAX_WORDS];                // per fetched word k: its column in the block ...
    uint64_t out_off[GGRS_QUERY_MAX_WORDS];                // ... and in the output buffer
    uint64_t* unit_match; uint64_t* unit_off;
    uint32_t col_ts[GGRS_QUERY_MAX_WORDS];
    uint32_t n_units, n_masks, without, n_words, slots;
    uint8_t col_wb[GGRS_QUERY_MAX_WORDS];
};
__device__ __forceinline__ void query_store(uint8_t* p, uint64_t v, uint32_t wb) {
    switch (wb) {
    case 8: *reinterpret_cast<uint64_t*>(p) = v; break;
    case 4: *reinterpret_cast<uint32_t*>(p) = (uint32_t)v; break;
    case 2: *reinterpret_cast<uint16_t*>(p) = (uint16_t)v; break;
    default: *p = (uint8_t)v;
    }
}
__global__ __launch_bounds__(TPB) void k_query_match(QueryArgs a) {
    for (uint32_t u = blockIdx.x * TPB + threadIdx.x; u <= a.n_units; u += gridDim.x * TPB) {
        uint64_t m = 0;
        if (u < a.n_units) {
            m = *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + (uint64_t)u * 8u) & diff_len_mask(a.len, (uint64_t)u * 64u);
            for (uint32_t j = 0; j < a.n_masks; ++j) {
                const uint64_t p = *reinterpret_cast<const uint64_t*>(a.state + a.off_mask[j] + (uint64_t)u * 8u);
                m &= ((a.without >> j) & 1u) ? ~p : p;
            }
        }
        a.unit_match[u] = m;
    }
}
__global__ __launch_bounds__(TPB) void k_query_emit(QueryArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (uint32_t u = blockIdx.x * (TPB / 64) + wave; u < a.n_units; u += gridDim.x * (TPB / 64)) {
        const uint64_t m = a.unit_match[u], off = a.unit_off[u];
        if (!m || off >= a.max_rows) continue;                                   // (wave-uniform)
        const uint64_t e = (uint64_t)u * 64u + lane, row = off + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (!((m >> lane) & 1ull) || row >= a.max_rows) continue;                // (no ballot, no barrier below: the lanes need not meet again)
        for (uint32_t k0 = 0; k0 < a.n_words; k0 += QUERY_BATCH) {
            uint64_t v[QUERY_BATCH];
#pragma unroll
            for (uint32_t i = 0; i < QUERY_BATCH; ++i) {
                v[i] = 0;
                if (k0 + i < a.n_words) {                                        // (uniform)
                    const uint32_t wb = a.col_wb[k0 + i];
                    v[i] = diff_load(a.state + col_at(a.col_off[k0 + i], a.col_ts[k0 + i], wb, e), wb);   // e < len <= the capacity: inside the column
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < QUERY_BATCH; ++i)
                if (k0 + i < a.n_words) { const uint32_t wb = a.col_wb[k0 + i]; query_store(a.out + a.out_off[k0 + i] + row * wb, v[i], wb); }
        }
        if (a.slots) *reinterpret_cast<uint32_t*>(a.out + a.slots_off + row * 4u) = (uint32_t)e;
    }
}

// ------------------------------------------------------------------ SCATTER (ggrs_hip_scatter)
// The inverse of the query: rows of (slot, words..) in device memory, in the query's output layout, applied to the LIVE block.  Two launches, ordered by their
// boundary alone; the host waits once, for the record:
//   k_scatter_check  one row per lane, grid-stride.  Row i is bad iff its slot is at or beyond len or the slot of row i-1 is not smaller (it reads slots i-1 and i):
//                    what is left is strictly ascending, so no two rows name one slot and the outcome cannot depend on the geometry.  Bad rows are counted and the
//                    lowest is kept (a 64-bit atomic min, spelled as the max of the row's complement so that one clear to zero initialises the whole record), one
//                    atomic each per wave that saw any, behind a __ballot.
//   k_scatter_apply  reads the count with a wave-uniform load and returns at once when it is not zero: nothing is written, and no host round trip sits between the
//                    launches.  Otherwise one row per lane, grid-stride: the lane loads its slot, the alive word and (WRITE, INSERT, REMOVE) the named presence words
//                    of unit slot >> 6 -- the lanes of one unit load the same words -- and is applied, dead or absent by ITS OWN bits of them, which no other row
//                    edits (no two rows share a slot): the verdict is the one of the state before the call whatever the other waves have done so far.  An applied
//                    lane of WRITE / INSERT loads its input words, QUERY_BATCH columns ahead of the first store, and stores them through col_at.  Mask edits are
//                    64-bit no-return atomics, OR (INSERT) or AND (REMOVE, DESPAWN), issued only where the bit changes: rows of one unit may sit in different waves
//                    and workgroups, a plain read-modify-write would lose bits.  The counts: dead and absent rows by one __ballot + popcount per wave-iteration into
//                    a wave-uniform sum, one LDS add per wave and one global atomic add per workgroup that saw any; the applied rows are n_rows minus the two,
//                    taken on the host.  (One global atomic add per wave-iteration and count, all to one address, measured 13 x slower at 1 M rows: the two
//                    series are in profiles/scatter/README.md and DESIGN.md section 3.17.)
enum : uint32_t { SCAT_BAD = 0, SCAT_FIRST_BAD = 1, SCAT_DEAD = 2, SCAT_ABSENT = 3, SCAT_REC_WORDS = 4 };   // the record, u64 words (SCAT_FIRST_BAD: ~row)
struct ScatterArgs {
    uint8_t* state; const uint8_t* in;
    unsigned long long* rec;
    uint64_t len, n_rows, off_alive, slots_off;
    uint64_t off_mask[MAX_COMPS];                          // presence masks: WRITE the named words' components (all must be present), INSERT / REMOVE the edited ones
    uint64_t col_off[GGRS_QUERY_MAX_WORDS];                // per word k: its column in the live block ...
    uint64_t in_off[GGRS_QUERY_MAX_WORDS];                 // ... and in the input buffer
    uint32_t col_ts[GGRS_QUERY_MAX_WORDS];
    uint32_t op, n_masks, n_words, pad;
    uint8_t col_wb[GGRS_QUERY_MAX_WORDS];
};
__global__ __launch_bounds__(TPB) void k_scatter_check(ScatterArgs a) {
    const uint32_t* const slots = reinterpret_cast<const uint32_t*>(a.in + a.slots_off);
    const uint64_t stride = (uint64_t)gridDim.x * TPB, n_pad = (a.n_rows + 63u) & ~63ull;      // (whole waves stay in the loop: the ballot below is over all 64 lanes)
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n_pad; i += stride) {
        bool bad = false;
        if (i < a.n_rows) {
            const uint32_t s = slots[i];
            bad = s >= a.len || (i > 0 && slots[i - 1] >= s);
        }
        const uint64_t b = __ballot(bad);
        if (b && (threadIdx.x & 63u) == 0u) {                                     // (the wave's rows ascend with the lane: its lowest bad row is its lowest set bit)
            atomicAdd(a.rec + SCAT_BAD, (unsigned long long)__popcll(b));
            atomicMax(a.rec + SCAT_FIRST_BAD, ~(unsigned long long)(i + (uint64_t)__ffsll((long long)b) - 1u));
        }
    }
}
__global__ __launch_bounds__(TPB) void k_scatter_apply(ScatterArgs a) {
    if (a.rec[SCAT_BAD]) return;                                                 // (wave-uniform: the check launch found a bad row -- nothing is applied)
    const uint32_t* const slots = reinterpret_cast<const uint32_t*>(a.in + a.slots_off);
    const uint64_t stride = (uint64_t)gridDim.x * TPB, n_pad = (a.n_rows + 63u) & ~63ull;
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    __shared__ unsigned long long s_cnt[2];
    if (threadIdx.x < 2u) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint64_t n_dead = 0, n_absent = 0;                                           // (wave-uniform)
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n_pad; i += stride) {
        const bool row = i < a.n_rows;
        uint64_t e = 0, bit = 0, alive = 0, have = ~0ull, wi = 0;
        if (row) {
            e = slots[i]; wi = (e >> 6) * 8u; bit = 1ull << (e & 63u);              // e < len <= the capacity (k_scatter_check): inside every mask and column
            alive = *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + wi) & bit;
        }
        const bool dead = row && !alive;
        bool absent = false;
        if (row && alive && a.op == GGRS_SCATTER_WRITE) {
            for (uint32_t j = 0; j < a.n_masks; ++j) have &= *reinterpret_cast<const uint64_t*>(a.state + a.off_mask[j] + wi);
            absent = !(have & bit);
        }
        const bool on = row && alive && !absent;
        if (on && a.op <= GGRS_SCATTER_INSERT) {
            for (uint32_t k0 = 0; k0 < a.n_words; k0 += QUERY_BATCH) {
                uint64_t v[QUERY_BATCH];
#pragma unroll
                for (uint32_t q = 0; q < QUERY_BATCH; ++q) {
                    v[q] = 0;
                    if (k0 + q < a.n_words) { const uint32_t wb = a.col_wb[k0 + q]; v[q] = diff_load(a.in + a.in_off[k0 + q] + i * wb, wb); }   // (uniform)
                }
#pragma unroll
                for (uint32_t q = 0; q < QUERY_BATCH; ++q)
                    if (k0 + q < a.n_words) { const uint32_t wb = a.col_wb[k0 + q]; query_store(a.state + col_at(a.col_off[k0 + q], a.col_ts[k0 + q], wb, e), v[q], wb); }
            }
        }
        if (on && a.op == GGRS_SCATTER_INSERT) {
            for (uint32_t j = 0; j < a.n_masks; ++j) {
                unsigned long long* const p = reinterpret_cast<unsigned long long*>(a.state + a.off_mask[j] + wi);
                if (!(*p & bit)) (void)atomicOr(p, (unsigned long long)bit);
            }
        } else if (on && a.op == GGRS_SCATTER_REMOVE) {
            for (uint32_t j = 0; j < a.n_masks; ++j) {
                unsigned long long* const p = reinterpret_cast<unsigned long long*>(a.state + a.off_mask[j] + wi);
                if (*p & bit) (void)atomicAnd(p, (unsigned long long)~bit);
            }
        } else if (on && a.op == GGRS_SCATTER_DESPAWN) {
            (void)atomicAnd(reinterpret_cast<unsigned long long*>(a.state + a.off_alive + wi), (unsigned long long)~bit);      // (on: the bit is set)
        }
        n_dead += (uint64_t)__popcll(__ballot(dead)); n_absent += (uint64_t)__popcll(__ballot(absent));
    }
    if (lane0) {
        if (n_dead) atomicAdd(&s_cnt[0], (unsigned long long)n_dead);
        if (n_absent) atomicAdd(&s_cnt[1], (unsigned long long)n_absent);
    }
    __syncthreads();
    if (threadIdx.x < 2u && s_cnt[threadIdx.x]) atomicAdd(a.rec + SCAT_DEAD + threadIdx.x, s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------------ DELTA (ggrs_hip_delta_frames / ggrs_hip_delta_block)
// Query<.., Changed<C>> / Added<C> / RemovedComponents<C> / despawns between TWO packed blocks: the query's stream compaction with a predicate that looks at both
// sides.  The BASE side is the one rows are fetched from and the filter is judged on (NEW for CHANGED and ADDED, OLD for REMOVED and DESPAWNED); the OTHER side only
// says what was there.  A_x(s): s below the side's len and alive; P_x(c, s): A_x(s) and component c present.  With F the query's match word on the base side:
//   ADDED / REMOVED   F & OR_c (P_base(c) & ~P_other(c))          DESPAWNED   F & ~A_other          CHANGED   F & OR_c (P_base(c) & (~P_other(c) | a word of c differs))
// One match launch, then k_diff_scan and k_query_emit as they are, over the base side (no compare-and-swap, no wait between workgroups, no atomic at all):
//   k_delta_match_masks   ADDED, REMOVED, DESPAWNED need mask words only: one 64-slot unit per LANE as in k_query_match, every mask of both sides one coalesced load.
//   k_delta_match_values  CHANGED: one unit per wave-iteration, one slot per lane.  The mask words are wave-uniform loads and F comes first; per component
//                         added = P_new & ~P_old joins the match word without a column being read, and the component's columns are read only while
//                         common & F & ~match has a bit left (tile-major through col_at, DIFF_BATCH columns of both sides in flight before the first __ballot).
//                         A unit whose match word has reached F reads nothing more.  Lane 0 stores the word.
// Both store a zero sentinel behind the last unit: the scan's word there is the number of matches.
struct DeltaArgs {
    const uint8_t* base; const uint8_t* other;
    uint64_t len_base, len_other, off_alive;
    uint64_t off_mask[MAX_COMPS];                          // presence masks of q's filtered components on the base side (bit j of without says which way)
    uint64_t off_present[MAX_COMPS];                       // per component j of changed_mask
    uint64_t col_off[DIFF_MAX_COLS];                       // per compared column (grouped by component)
    uint64_t* unit_match;
    uint32_t col_ts[DIFF_MAX_COLS];
    uint32_t n_units, n_masks, without, n_comps, kind;
    uint8_t comp_col0[MAX_COMPS], comp_ncols[MAX_COMPS];   // a component's first compared column and how many (0: the host knows its words are equal)
    uint8_t col_wb[DIFF_MAX_COLS];
};
__global__ __launch_bounds__(TPB) void k_delta_match_masks(DeltaArgs a) {
    for (uint32_t u = blockIdx.x * TPB + threadIdx.x; u <= a.n_units; u += gridDim.x * TPB) {
        uint64_t m = 0;
        if (u < a.n_units) {                                                     // (u < n_units <= the padded capacity / 64: inside every mask of both blocks)
            const uint64_t lo = (uint64_t)u * 64u, wo = (uint64_t)u * 8u;
            const uint64_t ab = *reinterpret_cast<const uint64_t*>(a.base + a.off_alive + wo) & diff_len_mask(a.len_base, lo);
            const uint64_t ao = *reinterpret_cast<const uint64_t*>(a.other + a.off_alive + wo) & diff_len_mask(a.len_other, lo);
            uint64_t f = ab;
            for (uint32_t j = 0; j < a.n_masks; ++j) {
                const uint64_t p = *reinterpret_cast<const uint64_t*>(a.base + a.off_mask[j] + wo);
                f &= ((a.without >> j) & 1u) ? ~p : p;
            }
            if (a.kind == GGRS_DELTA_DESPAWNED) m = f & ~ao;
            else {
                uint64_t acc = 0;
                for (uint32_t j = 0; j < a.n_comps; ++j) {
                    const uint64_t pb = *reinterpret_cast<const uint64_t*>(a.base + a.off_present[j] + wo);
                    const uint64_t po = *reinterpret_cast<const uint64_t*>(a.other + a.off_present[j] + wo) & ao;
                    acc |= pb & ~po;
                }
                m = f & acc;                                                     // (f is inside the base's alive word: pb needs no cut of its own)
            }
        }
        a.unit_match[u] = m;
    }
}
__global__ __launch_bounds__(TPB) void k_delta_match_values(DeltaArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (uint32_t u = blockIdx.x * (TPB / 64) + wave; u <= a.n_units; u += gridDim.x * (TPB / 64)) {
        uint64_t match = 0;
        if (u < a.n_units) {                                                     // (wave-uniform, as everything below that decides a branch)
            const uint64_t lo = (uint64_t)u * 64u, e = lo + lane, wo = (uint64_t)u * 8u;
            const uint64_t ab = *reinterpret_cast<const uint64_t*>(a.base + a.off_alive + wo) & diff_len_mask(a.len_base, lo);
            const uint64_t ao = *reinterpret_cast<const uint64_t*>(a.other + a.off_alive + wo) & diff_len_mask(a.len_other, lo);
            uint64_t f = ab;
            for (uint32_t j = 0; j < a.n_masks; ++j) {
                const uint64_t p = *reinterpret_cast<const uint64_t*>(a.base + a.off_mask[j] + wo);
                f &= ((a.without >> j) & 1u) ? ~p : p;
            }
            for (uint32_t j = 0; j < a.n_comps && match != f; ++j) {
                const uint64_t pb = *reinterpret_cast<const uint64_t*>(a.base + a.off_present[j] + wo) & f;
                const uint64_t po = *reinterpret_cast<const uint64_t*>(a.other + a.off_present[j] + wo) & ao;
                const uint64_t added = pb & ~po, common = pb & po;
                match |= added;
                const uint32_t q1 = (uint32_t)a.comp_col0[j] + a.comp_ncols[j];
                for (uint32_t q0 = a.comp_col0[j]; q0 < q1 && (common & ~match); q0 += DIFF_BATCH) {   // nobody left to decide -> the columns are not read
                    uint64_t va[DIFF_BATCH], vb[DIFF_BATCH];
#pragma unroll
                    for (uint32_t i = 0; i < DIFF_BATCH; ++i) {
                        va[i] = 0; vb[i] = 0;
                        if (q0 + i < q1) {
                            const uint32_t wb = a.col_wb[q0 + i];
                            const uint64_t off = col_at(a.col_off[q0 + i], a.col_ts[q0 + i], wb, e);   // e < the padded capacity: inside the column for every lane
                            va[i] = diff_load(a.base + off, wb); vb[i] = diff_load(a.other + off, wb);
                        }
                    }
#pragma unroll
                    for (uint32_t i = 0; i < DIFF_BATCH; ++i) match |= __ballot(va[i] != vb[i]) & common;   // (a column beyond the component's last: 0 != 0 for nobody)
                }
            }
        }
        if (lane == 0) a.unit_match[u] = match;
    }
}

// ------------------------------------------------------------------ SORTED QUERY (ggrs_hip_query_sorted / ggrs_hip_query_sorted_block)
// query.iter().sort_by(..) over one packed block: the query's rows, ordered by up to GGRS_SORT_MAX_KEYS key words instead of by slot.  k_query_match and k_diff_scan
// as they are; the host reads the number of matches (the radix launches take n and n_tiles by value); then
//   k_sort_rows    one 64-slot unit per wave-iteration, as k_query_emit walks them: a matching lane stores its slot at val[row] and the least significant stage's
//                  transformed key at key[row], for ALL matching rows (max_rows cuts the emit, not the sort).
//   the stages     least significant first.  A stage is one 32-bit key: a key word of up to 4 bytes is one stage, an 8-byte word two (low half, then high half).
//                  The transform is taken at the word's width before it is split: U the bits, I the bits ^ the sign bit, F the bits ^ (sign set ? all ones : the
//                  sign bit) -- IEEE-754 total order --, DESC the complement of that.  Every stage but the first begins with k_sort_rekey (key[i] = the transformed
//                  word of slot val[i]: a gather through col_at); then k_ix_hist<false> / k_ix_scan / k_ix_scatter<false> as they are, one pass per byte of the
//                  stage, ping-ponging two key and two val arrays.  The passes are stable, the rows start in slot order: stability gives the precedence of the
//                  keys and the ascending-slot tie-break, also under DESC.
//   k_sort_small   at most IX_TILE matches: ONE workgroup does every stage in one launch, from the tile bodies as ix_small_pass uses them, the rekey between the
//                  stages inside the launch; a workgroup fence and a barrier stand where the large form has a kernel boundary.
//   k_sort_emit    one row per lane, grid-stride over [0, n_rows): slot = val[row]; the fetched words are gathered through col_at, QUERY_BATCH columns' loads ahead of
//                  the first store, and stored at `row`, coalesced; the slots column is val[row].
// No compare-and-swap, no wait between workgroups, no position from an atomic's return value; plain vector loads and stores.
constexpr uint32_t SORT_MAX_STAGES = 2 * GGRS_SORT_MAX_KEYS;
struct SortStage { uint64_t col_off; uint32_t col_ts, passes; uint8_t wb, kind, desc, half; uint32_t pad; };   // passes: the radix passes of this stage (1, 2 or 4)
struct SortArgs {
    const uint8_t* state;
    uint32_t* key[2]; uint32_t* val[2];                    // the ping-pong pairs: k_sort_rows fills [0]
    uint64_t n;                                            // the matching rows: every one of them is sorted
    uint32_t n_stages, pad;
    SortStage st[SORT_MAX_STAGES];
};
// the order-preserving unsigned image of the key word of slot e, at the word's width, and the stage's 32 bits of it
__device__ __forceinline__ uint32_t sort_stage_key(const uint8_t* state, const SortStage& s, uint64_t e) {
    const uint32_t wb = s.wb, bits = 8u * wb;
    const uint64_t v = diff_load(state + col_at(s.col_off, s.col_ts, wb, e), wb);          // e < len <= the capacity: inside the column
    const uint64_t mask = ~0ull >> (64u - bits), sign = 1ull << (bits - 1u);
    uint64_t t = v;
    if (s.kind == GGRS_SORT_I) t = v ^ sign;
    else if (s.kind == GGRS_SORT_F) t = v ^ ((v & sign) ? mask : sign);
    if (s.desc) t = ~t & mask;
    return (uint32_t)(s.half ? t >> 32 : t);
}
__global__ __launch_bounds__(TPB) void k_sort_rows(QueryArgs a, SortArgs s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    for (uint32_t u = blockIdx.x * (TPB / 64) + wave; u < a.n_units; u += gridDim.x * (TPB / 64)) {
        const uint64_t m = a.unit_match[u];
        if (!((m >> lane) & 1ull)) continue;
        const uint64_t e = (uint64_t)u * 64u + lane, row = a.unit_off[u] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));   // row < n: the scan's total
        s.val[0][row] = (uint32_t)e;
        s.key[0][row] = sort_stage_key(a.state, s.st[0], e);
    }
}
__device__ __forceinline__ void sort_rekey(const SortArgs& s, const SortStage& st, uint32_t* key, const uint32_t* val, uint64_t first, uint64_t stride) {
    for (uint64_t i = first; i < s.n; i += stride) key[i] = sort_stage_key(s.state, st, val[i]);
}
__global__ __launch_bounds__(TPB) void k_sort_rekey(SortArgs s, uint32_t stage, uint32_t cur) {
    sort_rekey(s, s.st[stage], s.key[cur], s.val[cur], (uint64_t)blockIdx.x * TPB + threadIdx.x, (uint64_t)gridDim.x * TPB);
}
__global__ __launch_bounds__(IX_TPB) void k_sort_small(SortArgs s) {
    __shared__ uint32_t h[256], tab[256], base[256], cnt[IX_TPB / 64][256];
    uint32_t cur = 0;
    for (uint32_t g = 0; g < s.n_stages; ++g) {
        if (g) {                                                                 // (the vals were stored by other waves of this workgroup: the pass ended on a fence and a barrier)
            sort_rekey(s, s.st[g], s.key[cur], s.val[cur], threadIdx.x, IX_TPB);
            __threadfence_block();
            __syncthreads();
        }
        for (uint32_t p = 0; p < s.st[g].passes; ++p, cur ^= 1u) {
            IxArgs a;
            a.key_col = nullptr; a.vis = nullptr; a.key_in = s.key[cur]; a.val_in = s.val[cur]; a.key_out = s.key[cur ^ 1u]; a.val_out = s.val[cur ^ 1u]; a.hist = nullptr;
            a.n = s.n; a.n_tiles = 1; a.n_buckets = 0; a.shift = 8u * p;
            ix_small_pass<false>(a, h, tab, base, cnt);
        }
    }
}
__global__ __launch_bounds__(TPB) void k_sort_emit(QueryArgs a, const uint32_t* __restrict__ val, uint64_t n_rows) {
    const uint64_t stride = (uint64_t)gridDim.x * TPB;
    for (uint64_t row = (uint64_t)blockIdx.x * TPB + threadIdx.x; row < n_rows; row += stride) {
        const uint64_t e = val[row];                                             // a slot k_sort_rows stored: below len
        for (uint32_t k0 = 0; k0 < a.n_words; k0 += QUERY_BATCH) {
            uint64_t v[QUERY_BATCH];
#pragma unroll
            for (uint32_t i = 0; i < QUERY_BATCH; ++i) {
                v[i] = 0;
                if (k0 + i < a.n_words) {                                        // (uniform)
                    const uint32_t wb = a.col_wb[k0 + i];
                    v[i] = diff_load(a.state + col_at(a.col_off[k0 + i], a.col_ts[k0 + i], wb, e), wb);
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < QUERY_BATCH; ++i)
                if (k0 + i < a.n_words) { const uint32_t wb = a.col_wb[k0 + i]; query_store(a.out + a.out_off[k0 + i] + row * wb, v[i], wb); }
        }
        if (a.slots) *reinterpret_cast<uint32_t*>(a.out + a.slots_off + row * 4u) = (uint32_t)e;
    }
}
// ------------------------------------------------------------------ END OF SORTED QUERY

}  // namespace ggrs