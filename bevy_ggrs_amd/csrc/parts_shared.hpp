// parts_shared.hpp -- the device code of the CHECKSUM PARTS pass (ggrs_hip_checksum_parts) that its two hashing kernels have in common: the statically compiled
// k_parts_hash (kernels.hpp includes this file as code) and ggrs_jit_parts, the kernel generated for a world with a user-written hasher (kernel_gen.hpp includes
// it as a string, behind device_prelude.hpp).  One text: the argument block, the accumulator rows and the way they leave a workgroup cannot drift between the two.
// The whole body is the argument of GGRS_SHARED_CODE(...), as in device_prelude.hpp: comments are fine, preprocessor directives are not.
// Nothing the tick's generated text includes is touched by this file.
GGRS_SHARED_CODE(
constexpr int PARTS_MAX = 32;                              // checksum specs of a world (GGRS_MAX_COMPONENTS)
constexpr int PARTS_WAVES = 4;                             // waves of a workgroup
constexpr int PARTS_CELLS = 2 * PARTS_MAX + 1;             // an accumulator row: cell k the XOR of spec k, n_cks + k its n_hashed, 2 n_cks the live count
constexpr int PARTS_STRIPES = 32;                          // copies of the row in device memory: a workgroup adds into copy `workgroup index mod PARTS_STRIPES`, so that thousands
constexpr int PARTS_STRIPE_CELLS = 72;                     // of workgroups do not queue on one cache line (a copy starts on a 64-byte line of its own: 72 x 8 bytes)
struct PartsWord { uint64_t off; uint32_t wb; uint32_t ts; };   // one hashed word: slot e's word of wb bytes at parts_col_at(off, ts, wb, e)
struct PartsArgs {
    const uint8_t* state;                                  // a complete packed block
    const PartsWord* words;                                // the specs' hashed words, spec k's at [word_base[k], word_base[k] + n_words[k])  (k_parts_hash only)
    unsigned long long* acc;                               // PARTS_STRIPES rows of PARTS_STRIPE_CELLS cells, zeroed ahead of the launch
    uint64_t len, off_alive;
    uint32_t n_units, n_cks;                               // 64-slot units of [0, len); checksum specs
    uint64_t off_present[PARTS_MAX];
    uint32_t n_words[PARTS_MAX], word_base[PARTS_MAX];
};
__device__ __forceinline__ uint64_t parts_col_at(uint64_t col_off, uint32_t tile_stride, uint32_t word_bytes, uint64_t e) {
    return col_off + (e >> LT_SHIFT) * (uint64_t)tile_stride + (e & (uint64_t)(LAYOUT_TILE - 1)) * (uint64_t)word_bytes;
}
__device__ __forceinline__ uint64_t parts_load(const uint8_t* p, uint32_t wb) {
    switch (wb) {
    case 8: return *reinterpret_cast<const uint64_t*>(p);
    case 4: return *reinterpret_cast<const uint32_t*>(p);
    case 2: return *reinterpret_cast<const uint16_t*>(p);
    default: return *p;
    }
}
// the alive word of unit u, cut by len: a slot at or beyond len is dead whatever its mask bit says.  A wave-uniform load
__device__ __forceinline__ uint64_t parts_alive(const PartsArgs& a, uint32_t u) {
    const uint64_t lo = (uint64_t)u * 64u;
    const uint64_t cut = a.len >= lo + 64u ? ~0ull : (a.len > lo ? (1ull << (a.len - lo)) - 1ull : 0ull);
    return *reinterpret_cast<const uint64_t*>(a.state + a.off_alive + (uint64_t)u * 8u) & cut;
}
__device__ __forceinline__ uint64_t parts_present(const PartsArgs& a, uint32_t k, uint32_t u) { return *reinterpret_cast<const uint64_t*>(a.state + a.off_present[k] + (uint64_t)u * 8u); }
// the accumulator rows, one per wave, in LDS: a wave is the only writer of its row, so lane 0 updates it with plain reads and writes
__device__ __forceinline__ void parts_rows_clear(unsigned long long* s_rows) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)(PARTS_WAVES * PARTS_CELLS); i += 256u) s_rows[i] = 0ull;
    __syncthreads();
}
// spec k of one unit: every lane's entity hash (0 where the entity is dead or lacks the component) becomes the wave's XOR; m = alive & present of the unit
__device__ __forceinline__ void parts_put(unsigned long long* row, uint32_t n_cks, uint32_t k, uint64_t h, uint64_t m, uint32_t lane) {
    h = wave_xor(h);
    if (lane == 0u) { row[k] ^= h; row[n_cks + k] += (unsigned long long)__popcll(m); }
}
// the rows of the workgroup's waves combined; every non-zero cell leaves with ONE 64-bit atomic per workgroup -- XOR for the hashes, add for the counts: both are
// order-free, so the result cannot depend on the grid (nor on which copy of the row a workgroup adds into: k_parts_finish folds the copies).  No ticket, no wait
// between workgroups: k_parts_finish runs behind the launch's boundary
__device__ __forceinline__ void parts_rows_flush(const PartsArgs& a, const unsigned long long* s_rows) {
    __syncthreads();
    const uint32_t i = threadIdx.x;
    if (i > 2u * a.n_cks) return;
    unsigned long long v = 0ull;
    if (i < a.n_cks) { for (int wv = 0; wv < PARTS_WAVES; ++wv) v ^= s_rows[wv * PARTS_CELLS + i]; }
    else { for (int wv = 0; wv < PARTS_WAVES; ++wv) v += s_rows[wv * PARTS_CELLS + i]; }
    if (!v) return;
    unsigned long long* const cell = a.acc + (blockIdx.x % (uint32_t)PARTS_STRIPES) * (uint32_t)PARTS_STRIPE_CELLS + i;
    if (i < a.n_cks) (void)__hip_atomic_fetch_xor(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else (void)__hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
)
