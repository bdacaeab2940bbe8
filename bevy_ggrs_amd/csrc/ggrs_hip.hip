// ggrs_hip.hip -- libggrs_hip.so: host runtime + C ABI (see include/ggrs_hip.h).  ONE translation unit, in parts:
//   kernels.hpp / device_prelude.hpp   gfx950 device code (the per-request kernels, the checksum folds, the text shared with generated kernels)
//   host_world.hpp                     struct ggrs_world, knobs, layout of a packed state block, row versions
//   kernel_gen.hpp                     hiprtc plumbing, custom systems, the per-world request-group kernel generator, module cache
//   host_seal.hpp                      sealing: fused-path recognition, kernel generation, arena carve
//   host_requests.hpp                  one launch per request (SaveWorld / LoadWorld / AdvanceWorld), ring, spawns, host-side fold
//   host_groups.hpp                    fused request groups: run_request_groups_gen
//   host_fanout.hpp                    speculative fan-out over RCCL (ggrs_hip_fanout_*)
//   this file                          the C ABI entry points
//
// One ggrs_world owns: a device arena carved into identical *packed state blocks* (one live block + up to max_depth ring
// slots), the host-side ring bookkeeping (an exact mirror of GgrsSnapshots<_, _>, /root/reference/src/snapshot/mod.rs:121-243,
// over slot indices instead of HashMaps), the registered component/system tables and one HIP stream.  Every request becomes
// kernel launches on that stream; the only host<->device synchronisation in handle_requests is one checksum read-back at the
// end of the batch.
//
// There is NO CPU fallback: without a HIP device world creation fails with GGRS_E_NO_DEVICE.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>      // hipExtModuleLaunchKernel: event pairs that ride on a dispatch (profiling)
#include <hip/hiprtc.h>   // types and prototypes only: resolved with dlsym on first use (no link-time dependency)
#include <rccl/rccl.h>      // types and prototypes only: every entry point is resolved with dlsym (no link-time dependency)
#include <dlfcn.h>
#include <math.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <cctype>
#include <chrono>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/ggrs_hip.h"
#include "kernels.hpp"

using namespace ggrs;

#include "host_world.hpp"
namespace {
#include "kernel_gen.hpp"
}
#include "host_seal.hpp"
#include "host_requests.hpp"
#include "host_groups.hpp"

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int ggrs_hip_abi_version(void) { return GGRS_HIP_ABI_VERSION; }
int ggrs_hip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }

int ggrs_hip_world_create_ex(const ggrs_world_desc* d, ggrs_world** out) {
    if (!d || !out || d->capacity == 0 || d->capacity > (1ULL << 28)) return GGRS_E_INVALID;   // 32-bit lane offsets in the kernels
    if (d->flags & GGRS_WORLD_LAYOUT_ONLY) {
        ggrs_world* w = new ggrs_world();
        w->layout_only = true;
        w->device = d->device; w->capacity = d->capacity; w->cap_pad = align_up(d->capacity, LAYOUT_TILE);
        w->max_depth = d->max_depth ? d->max_depth : 8; w->flags = d->flags; w->depth = w->max_depth;
        w->knobs = Knobs::from_env();
        *out = w;
        return GGRS_OK;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || d->device >= n) return GGRS_E_NO_DEVICE;
    if (hipSetDevice(d->device) != hipSuccess) return GGRS_E_NO_DEVICE;
    ggrs_world* w = new ggrs_world();
    w->device = d->device; w->capacity = d->capacity; w->cap_pad = align_up(d->capacity, LAYOUT_TILE);
    w->max_depth = d->max_depth ? d->max_depth : 8; w->flags = d->flags;
    w->depth = w->max_depth;
    w->nt_copy = (d->flags & GGRS_WORLD_NT_COPY) != 0;
    w->knobs = Knobs::from_env();
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d->device) == hipSuccess && v > 0) w->n_cu = v; }
    if (d->stream) w->stream = (hipStream_t)d->stream;
    else {
        if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; return GGRS_E_HIP; }
        w->own_stream = true;
    }
    if (d->arena && d->arena_bytes) { w->arena = (uint8_t*)d->arena; w->arena_bytes = d->arena_bytes; }
    *out = w;
    return GGRS_OK;
}
int ggrs_hip_world_create(int device, uint64_t capacity, uint32_t max_depth, ggrs_world** out) {
    ggrs_world_desc d; memset(&d, 0, sizeof d);
    d.device = device; d.capacity = capacity; d.max_depth = max_depth;
    return ggrs_hip_world_create_ex(&d, out);
}
uint64_t ggrs_hip_arena_bytes(uint64_t capacity, uint32_t max_depth, uint32_t n_components, uint32_t bytes_per_slot) {
    const uint64_t cap_pad = align_up(capacity, LAYOUT_TILE);
    const uint64_t mask = align_up(cap_pad / 8, ALIGN);
    // header + liveness/presence masks, 4 KiB aligned, then the tile-major word columns (bytes_per_slot x 8192 per layout tile; for a component
    // under a Strategy count its Stored words too)
    // ... and the value tags: one u32 per 64-slot unit and word column (at most one column per registered byte)
    const uint64_t state = align_up(align_up(align_up(ALIGN + (1 + (uint64_t)n_components) * mask, 4096) + cap_pad * bytes_per_slot, ALIGN) + (cap_pad / 64) * 4ull * bytes_per_slot, 4096);
    const uint64_t parts = align_up((uint64_t)(n_components + 1) * (cap_pad / TILE + 4096) * 8, ALIGN);
    const uint64_t side = align_up(mask + align_up(cap_pad * 4, ALIGN) + (uint64_t)n_components * mask + cap_pad * bytes_per_slot + (uint64_t)(bytes_per_slot + 1) * ALIGN, 4096);
    // + checksum units, mask scratch, the spawn staging buffer's device twin (GGRS_STAGE_BYTES, default 8 MiB; at most 1 GiB is accounted for here)
    const Knobs k = Knobs::from_env();
    return (uint64_t)(max_depth + 1) * state + side + parts + (uint64_t)(GGRS_MAX_COMPONENTS * GGRS_MAX_CKS_UNITS + 1) * sizeof(UnitDesc) + ALIGN * 4 + k.stage_bytes + 2 * ALIGN;
}
void ggrs_hip_world_destroy(ggrs_world* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->fanout_backref) *w->fanout_backref = nullptr;          // a ggrs_fanout destroyed after its world (interpreter shutdown order) finds no world
    for (auto& e : w->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (hipEvent_t e : w->prof_pool) (void)hipEventDestroy(e);
    for (auto& b : w->pending) (void)hipEventDestroy(b.ev);
    for (auto& e : w->event_pool) (void)hipEventDestroy(e);
    for (auto& e : w->ff_events) if (e.ev) (void)hipEventDestroy(e.ev);
    for (auto& c : w->customs) if (c.mod) (void)hipModuleUnload(c.mod);
    jit_spec_retire(w);
    jit_release(w->jit_entry);
    delete w->jl; w->jl = nullptr;
    if (w->d_gen_parts) (void)hipFree(w->d_gen_parts);
    if (w->d_branch_parts) (void)hipFree(w->d_branch_parts);
    if (w->d_branch_marks) (void)hipFree(w->d_branch_marks);
    if (w->d_branch_gone) (void)hipFree(w->d_branch_gone);
    if (w->d_skip) (void)hipFree(w->d_skip);
    if (w->d_diff) (void)hipFree(w->d_diff);
    if (w->h_diff) (void)hipHostFree(w->h_diff);
    if (w->d_cparts) (void)hipFree(w->d_cparts);
    if (w->h_cparts) (void)hipHostFree(w->h_cparts);
    for (hipEvent_t e : w->cparts_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : w->query_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : w->scatter_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : w->sort_ev) if (e) (void)hipEventDestroy(e);
    jit_release(w->cparts_entry);
    sp_release(w);
    peer_view_release(w);
    fx_inbox_release(w);
    rd_inbox_release(w);
    sum_part_release(w);
    rx_inbox_release(w);
    rv_inbox_release(w);
    for (void* p : w->spec_allocs) (void)hipFree(p);
    if (w->h_results) (void)hipHostFree(w->h_results);
    if (w->h_stage) (void)hipHostFree(w->h_stage);
    if (w->h_rows) (void)hipHostFree(w->h_rows);
    arena_release(w);
    if (w->own_stream && w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}
int ggrs_hip_specialise_wait(ggrs_world* w) {
    if (!w) return GGRS_E_INVALID;
    int ready = 0;
    for (auto& s : w->spec_tab) {
        if (!s.spec) continue;
        if (s.spec->th.joinable()) s.spec->th.join();
        if (s.spec->state.load(std::memory_order_acquire) == 2) ready = 1;
    }
    return ready;
}
const char* ggrs_hip_last_error(ggrs_world* w) { return w ? w->err.c_str() : "null world"; }

int ggrs_hip_register_component(ggrs_world* w, const char* name, uint32_t word_bytes, uint32_t n_words, uint32_t* comp_id) {
    if (!w || !name) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "register_component after the world was sealed");
    if (w->comps.size() >= GGRS_MAX_COMPONENTS) return w->fail(GGRS_E_INVALID, "at most %d components per world (GGRS_MAX_COMPONENTS)", GGRS_MAX_COMPONENTS);
    if (n_words == 0 || n_words > GGRS_MAX_WORDS || (word_bytes != 1 && word_bytes != 2 && word_bytes != 4 && word_bytes != 8))
        return w->fail(GGRS_E_INVALID, "bad component shape (word_bytes must be 1, 2, 4 or 8; 1..%d words)", GGRS_MAX_WORDS);
    Comp c; c.name = name; c.word_bytes = word_bytes; c.n_words = n_words;
    c.defaults.assign((size_t)word_bytes * n_words, 0);
    w->comps.push_back(c);
    if (comp_id) *comp_id = (uint32_t)w->comps.size() - 1;
    return GGRS_OK;
}
int ggrs_hip_register_component_ex(ggrs_world* w, const char* name, uint32_t word_bytes, uint32_t n_words, uint32_t flags, uint32_t* comp_id) {
    if (flags & ~GGRS_COMP_NO_ROLLBACK) return w ? w->fail(GGRS_E_INVALID, "unknown component flags %u", flags) : GGRS_E_INVALID;
    uint32_t c = 0;
    const int rc = ggrs_hip_register_component(w, name, word_bytes, n_words, &c);
    if (rc) return rc;
    w->comps[c].no_rollback = (flags & GGRS_COMP_NO_ROLLBACK) != 0;
    if (comp_id) *comp_id = c;
    return GGRS_OK;
}
int ggrs_hip_set_component_default(ggrs_world* w, uint32_t c, const void* words) {
    if (!w || c >= w->comps.size() || !words) return GGRS_E_INVALID;
    memcpy(w->comps[c].defaults.data(), words, w->comps[c].defaults.size());
    return GGRS_OK;
}
int ggrs_hip_checksum_component(ggrs_world* w, uint32_t c, const uint32_t* word_idx, uint32_t n) {
    if (!w || c >= w->comps.size()) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "checksum_component after the world was sealed");
    Comp& cc = w->comps[c];
    if (n && !word_idx) return w->fail(GGRS_E_INVALID, "word list is NULL");
    cc.cks_words.clear(); cc.cks_source.clear();
    for (uint32_t k = 0; k < n; ++k) { if (word_idx[k] >= cc.n_words) return w->fail(GGRS_E_INVALID, "word index out of range"); cc.cks_words.push_back(word_idx[k]); }
    if (n > GGRS_MAX_CKS_UNITS) return w->fail(GGRS_E_INVALID, "checksum spec too long");
    cc.checksummed = true;
    return GGRS_OK;
}
int ggrs_hip_checksum_component_custom(ggrs_world* w, uint32_t c, const char* source) {
    if (!w || c >= w->comps.size() || !source || !*source) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "checksum_component after the world was sealed");
    Comp& cc = w->comps[c];
    if (cc.no_rollback) return w->fail(GGRS_E_INVALID, "component %u is not registered for rollback: it has no checksum", c);
    cc.cks_words.clear();
    cc.cks_source = source;
    cc.checksummed = true;
    return GGRS_OK;
}
int ggrs_hip_add_system(ggrs_world* w, const ggrs_system_desc* d) {
    if (!w || !d) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "add_system after the world was sealed");
    if (w->systems.size() >= GGRS_MAX_SYSTEMS) return w->fail(GGRS_E_INVALID, "too many systems");
    const uint32_t nc = (uint32_t)w->comps.size();
    auto comp_ok = [&](uint32_t c, uint32_t wb, uint32_t word, uint32_t span) { return c < nc && w->comps[c].word_bytes == wb && word + span <= w->comps[c].n_words; };
    bool ok = false;
    switch (d->kind) {
    case GGRS_SYS_PARTICLES_UPDATE: ok = comp_ok(d->comp[0], 4, d->word[0], 3) && comp_ok(d->comp[1], 4, d->word[1], 3); break;
    case GGRS_SYS_TTL_DESPAWN: ok = comp_ok(d->comp[0], 8, d->word[0], 1); break;
    case GGRS_SYS_PARTICLES_SPAWN: ok = comp_ok(d->comp[0], 4, 0, 3) && comp_ok(d->comp[1], 4, 0, 3) && comp_ok(d->comp[2], 8, 0, 1); break;
    case GGRS_SYS_ADD_U32: case GGRS_SYS_SAT_SUB_DESPAWN: ok = comp_ok(d->comp[0], 4, d->word[0], 1); break;
    case GGRS_SYS_BOX_MOVE: ok = comp_ok(d->comp[0], 4, d->word[0], 3) && comp_ok(d->comp[1], 4, d->word[1], 3) && comp_ok(d->comp[2], 8, d->word[2], 1); break;
    default: ok = false;
    }
    if (!ok) return w->fail(GGRS_E_INVALID, "system %u does not match the registered components", d->kind);
    w->systems.push_back(*d);
    return GGRS_OK;
}
int ggrs_hip_add_custom_system(ggrs_world* w, const ggrs_custom_system_desc* d) { return ggrs_hip_add_custom_system_peers(w, d, nullptr, 0); }
// ... with peer bindings: words of OTHER entities the system reads through e.peer(slot), as they were at the start of the frame (include/ggrs_hip.h)
int ggrs_hip_add_custom_system_peers(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers) { return ggrs_hip_add_custom_system_effects(w, d, peers, n_peers, nullptr, 0); }
// ... and with effect bindings: words of OTHER entities the system combines a value into through e.send_*(slot, j, v), landing at the end of the frame (include/ggrs_hip.h)
int ggrs_hip_add_custom_system_effects(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects) {
    return ggrs_hip_add_custom_system_commands(w, d, peers, n_peers, effects, n_effects, nullptr, 0);
}
// ... and with command bindings: whole components of its OWN entity the system sees as Option<&mut C> (e.has, e.opt_*) and may insert or remove (include/ggrs_hip.h)
int ggrs_hip_add_custom_system_commands(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                        const ggrs_command_binding* cmds, uint32_t n_cmds) {
    return ggrs_hip_add_custom_system_resources(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, nullptr, 0);
}
// ... and with resource bindings: words of the world's device resources the system reads through e.res_*(j), as they stand at that point of the frame (include/ggrs_hip.h)
int ggrs_hip_add_custom_system_resources(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                         const ggrs_command_binding* cmds, uint32_t n_cmds, const ggrs_resource_binding* res, uint32_t n_res) {
    return ggrs_hip_add_custom_system_reduces(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, res, n_res, nullptr, 0);
}
// ... and with reduce bindings: words of the world's device resources the system combines a value into through e.reduce_*(j, v), landing at the end of the frame
// (include/ggrs_hip.h).  Which resource, word and width a binding names is checked at seal (host_seal.hpp reduces_validate), with the registration-order rule
int ggrs_hip_add_custom_system_reduces(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                       const ggrs_command_binding* cmds, uint32_t n_cmds, const ggrs_resource_binding* res, uint32_t n_res, const ggrs_reduce_binding* red, uint32_t n_red) {
    return ggrs_hip_add_custom_system_remote(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, res, n_res, red, n_red, nullptr, 0);
}
// ... and with remote bindings: components of OTHER entities the system inserts or removes through e.send_insert / e.send_remove(slot, j), and e.send_despawn(slot),
// landing at the end of the frame (include/ggrs_hip.h).  The registration-order rules and what a component must be are checked at seal (host_seal.hpp remote_validate)
int ggrs_hip_add_custom_system_remote(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                      const ggrs_command_binding* cmds, uint32_t n_cmds, const ggrs_resource_binding* res, uint32_t n_res, const ggrs_reduce_binding* red, uint32_t n_red,
                                      const ggrs_remote_binding* rem, uint32_t n_rem) {
    return ggrs_hip_add_custom_system_sums(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, res, n_res, red, n_red, rem, n_rem, nullptr, 0);
}
// ... and with sum bindings: float / double words of the world's device resources the system adds into through e.sum_f32 / e.sum_f64(j, v), summed in a fixed order
// and landing at the end of the frame (include/ggrs_hip.h).  Which resource, word and width a binding names is checked at seal (host_seal.hpp sums_validate)
int ggrs_hip_add_custom_system_sums(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                    const ggrs_command_binding* cmds, uint32_t n_cmds, const ggrs_resource_binding* res, uint32_t n_res, const ggrs_reduce_binding* red, uint32_t n_red,
                                    const ggrs_remote_binding* rem, uint32_t n_rem, const ggrs_sum_binding* sum, uint32_t n_sum) {
    return ggrs_hip_add_custom_system_values(w, d, peers, n_peers, effects, n_effects, cmds, n_cmds, res, n_res, red, n_red, rem, n_rem, sum, n_sum, nullptr, 0);
}
// ... and with value bindings: components of OTHER entities the system inserts with ITS OWN words through e.val_*(j, k) / e.send_value(slot, j), the last sender in
// schedule order winning as one value, landing with the remote commands (include/ggrs_hip.h).  What a component must be is checked at seal (host_seal.hpp values_validate)
int ggrs_hip_add_custom_system_values(ggrs_world* w, const ggrs_custom_system_desc* d, const ggrs_peer_binding* peers, uint32_t n_peers, const ggrs_effect_binding* effects, uint32_t n_effects,
                                      const ggrs_command_binding* cmds, uint32_t n_cmds, const ggrs_resource_binding* res, uint32_t n_res, const ggrs_reduce_binding* red, uint32_t n_red,
                                      const ggrs_remote_binding* rem, uint32_t n_rem, const ggrs_sum_binding* sum, uint32_t n_sum, const ggrs_value_binding* val, uint32_t n_val) {
    if (!w || !d || !d->source) return GGRS_E_INVALID;
    if (n_val > GGRS_VALUE_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d value bindings (GGRS_VALUE_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_VALUE_MAX_BINDINGS, n_val);
    if (n_val && !val) return w->fail(GGRS_E_INVALID, "custom system: n_val = %u but val is NULL", n_val);
    if (n_sum > GGRS_SUM_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d sum bindings (GGRS_SUM_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_SUM_MAX_BINDINGS, n_sum);
    if (n_sum && !sum) return w->fail(GGRS_E_INVALID, "custom system: n_sum = %u but sum is NULL", n_sum);
    if (n_rem > GGRS_REMOTE_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d remote bindings (GGRS_REMOTE_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_REMOTE_MAX_BINDINGS, n_rem);
    if (n_rem && !rem) return w->fail(GGRS_E_INVALID, "custom system: n_rem = %u but rem is NULL", n_rem);
    if (n_red > GGRS_REDUCE_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d reduce bindings (GGRS_REDUCE_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_REDUCE_MAX_BINDINGS, n_red);
    if (n_red && !red) return w->fail(GGRS_E_INVALID, "custom system: n_red = %u but red is NULL", n_red);
    if (n_res > GGRS_RESOURCE_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d resource bindings (GGRS_RESOURCE_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_RESOURCE_MAX_BINDINGS, n_res);
    if (n_res && !res) return w->fail(GGRS_E_INVALID, "custom system: n_res = %u but res is NULL", n_res);
    if (n_cmds > GGRS_COMMAND_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system '%s': at most %d command bindings (GGRS_COMMAND_MAX_BINDINGS), not %u", d->name ? d->name : "custom", GGRS_COMMAND_MAX_BINDINGS, n_cmds);
    if (n_cmds && !cmds) return w->fail(GGRS_E_INVALID, "custom system: n_cmds = %u but cmds is NULL", n_cmds);
    if (w->sealed) return w->fail(GGRS_E_INVALID, "add_custom_system after the world was sealed");
    if (n_peers > GGRS_PEER_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system: at most %d peer bindings, not %u", GGRS_PEER_MAX_BINDINGS, n_peers);
    if (n_peers && !peers) return w->fail(GGRS_E_INVALID, "custom system: n_peers = %u but peers is NULL", n_peers);
    if (n_effects > GGRS_EFFECT_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system: at most %d effect bindings, not %u", GGRS_EFFECT_MAX_BINDINGS, n_effects);
    if (n_effects && !effects) return w->fail(GGRS_E_INVALID, "custom system: n_effects = %u but effects is NULL", n_effects);
    if (w->systems.size() >= GGRS_MAX_SYSTEMS) return w->fail(GGRS_E_INVALID, "too many systems");
    if (d->n_bindings == 0 || d->n_bindings > GGRS_CUSTOM_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "custom system: 1..%d bindings", GGRS_CUSTOM_MAX_BINDINGS);
    ggrs_world::Custom c;
    c.name = d->name ? d->name : "custom";
    c.n_bind = d->n_bindings;
    for (uint32_t i = 0; i < c.n_bind; ++i) {
        if (d->comp[i] >= w->comps.size() || d->word[i] >= w->comps[d->comp[i]].n_words)
            return w->fail(GGRS_E_INVALID, "custom system '%s': binding %u names word %u of component %u, which is not registered", c.name.c_str(), i, d->word[i], d->comp[i]);
        c.comp[i] = d->comp[i]; c.word[i] = d->word[i];
        bool seen = false;
        for (uint32_t p = 0; p < c.n_pres; ++p) seen |= c.pres_comp[p] == d->comp[i];
        if (!seen) c.pres_comp[c.n_pres++] = d->comp[i];
    }
    for (uint32_t j = 0; j < n_peers; ++j) {
        if (peers[j].comp >= w->comps.size() || peers[j].word >= w->comps[peers[j].comp].n_words)
            return w->fail(GGRS_E_INVALID, "custom system '%s': peer binding %u names word %u of component %u, which is not registered", c.name.c_str(), j, peers[j].word, peers[j].comp);
        c.pcomp[j] = peers[j].comp; c.pword[j] = peers[j].word;
    }
    c.n_peer = n_peers;
    for (uint32_t j = 0; j < n_effects; ++j) {
        if (effects[j].comp >= w->comps.size() || effects[j].word >= w->comps[effects[j].comp].n_words)
            return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u names word %u of component %u, which is not registered", c.name.c_str(), j, effects[j].word, effects[j].comp);
        if (effects[j].op > GGRS_EFFECT_XOR) return w->fail(GGRS_E_INVALID, "custom system '%s': effect binding %u has op %u, which is none of GGRS_EFFECT_*", c.name.c_str(), j, effects[j].op);
        c.fcomp[j] = effects[j].comp; c.fword[j] = effects[j].word; c.fop[j] = effects[j].op;
    }
    c.n_fx = n_effects;
    uint32_t cmd_words = 0;
    for (uint32_t j = 0; j < n_cmds; ++j) {
        if (cmds[j].comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "custom system '%s': command binding %u names component %u, which is not registered", c.name.c_str(), j, cmds[j].comp);
        if (cmds[j].flags & ~(GGRS_CMD_INSERT | GGRS_CMD_REMOVE)) return w->fail(GGRS_E_INVALID, "custom system '%s': command binding %u has flags %x, which are none of GGRS_CMD_*", c.name.c_str(), j, cmds[j].flags);
        c.ccomp[j] = cmds[j].comp; c.cflags[j] = cmds[j].flags;
        cmd_words += w->comps[cmds[j].comp].n_words;
    }
    if (cmd_words > GGRS_COMMAND_MAX_WORDS)
        return w->fail(GGRS_E_INVALID, "custom system '%s': its command-bound components have %u words together, at most %d (GGRS_COMMAND_MAX_WORDS)", c.name.c_str(), cmd_words, GGRS_COMMAND_MAX_WORDS);
    c.n_cmd = n_cmds;
    for (uint32_t j = 0; j < n_res; ++j) {
        if (res[j].res >= w->resources.size() || res[j].word >= w->resources[res[j].res].n_words)
            return w->fail(GGRS_E_INVALID, "custom system '%s': resource binding %u names word %u of resource %u, which is not registered", c.name.c_str(), j, res[j].word, res[j].res);
        c.rres[j] = res[j].res; c.rword[j] = res[j].word;
    }
    c.n_res = n_res;
    for (uint32_t j = 0; j < n_red; ++j) {
        if (red[j].op > GGRS_EFFECT_XOR) return w->fail(GGRS_E_INVALID, "custom system '%s': reduce binding %u (word %u of resource %u) has op %u, which is none of GGRS_EFFECT_*", c.name.c_str(), j, red[j].word, red[j].res, red[j].op);
        c.dres[j] = red[j].res; c.dword[j] = red[j].word; c.dop[j] = red[j].op;
    }
    c.n_red = n_red;
    for (uint32_t j = 0; j < n_rem; ++j) {
        const uint32_t fl = rem[j].flags;
        if (!fl || (fl & ~(GGRS_REMOTE_INSERT | GGRS_REMOTE_REMOVE | GGRS_REMOTE_DESPAWN))) return w->fail(GGRS_E_INVALID, "custom system '%s': remote binding %u has flags %x, which are none of GGRS_REMOTE_*", c.name.c_str(), j, fl);
        if (fl & GGRS_REMOTE_DESPAWN) {
            if (fl != GGRS_REMOTE_DESPAWN || rem[j].comp != GGRS_REMOTE_ENTITY)
                return w->fail(GGRS_E_INVALID, "custom system '%s': remote binding %u has GGRS_REMOTE_DESPAWN: such a binding names no component (comp = GGRS_REMOTE_ENTITY) and carries no other flag", c.name.c_str(), j);
        } else if (rem[j].comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "custom system '%s': remote binding %u names component %u, which is not registered", c.name.c_str(), j, rem[j].comp);
        for (uint32_t q = 0; q < j; ++q) if (c.xcomp[q] == rem[j].comp)
            return w->fail(GGRS_E_INVALID, "custom system '%s': remote bindings %u and %u name the same component %u: a component has one remote binding per system", c.name.c_str(), q, j, rem[j].comp);
        c.xcomp[j] = rem[j].comp; c.xflags[j] = fl;
    }
    c.n_rem = n_rem;
    for (uint32_t j = 0; j < n_sum; ++j) { c.sres[j] = sum[j].res; c.sword[j] = sum[j].word; }
    c.n_sum = n_sum;
    uint32_t val_words = 0;
    for (uint32_t j = 0; j < n_val; ++j) {
        if (val[j].comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "custom system '%s': value binding %u names component %u, which is not registered", c.name.c_str(), j, val[j].comp);
        if (val[j].flags) return w->fail(GGRS_E_INVALID, "custom system '%s': value binding %u (component %u, '%s') has flags %x: a value binding's flags must be 0", c.name.c_str(), j, val[j].comp, w->comps[val[j].comp].name.c_str(), val[j].flags);
        c.vcomp[j] = val[j].comp;
        val_words += w->comps[val[j].comp].n_words;
    }
    if (val_words > GGRS_VALUE_MAX_WORDS)
        return w->fail(GGRS_E_INVALID, "custom system '%s': its value bindings stage %u words together, at most %d (GGRS_VALUE_MAX_WORDS)", c.name.c_str(), val_words, GGRS_VALUE_MAX_WORDS);
    c.n_val = n_val;
    DeviceGuard dg(w);
    c.source = d->source;
    c.may_defer = source_has_token(c.source, "despawn_rollback") || source_has_token(c.source, "kill");
    const std::string src = custom_source(w, c, d->source);
    const std::string what = "custom system '" + c.name + "'";
    const int rc = hiprtc_build(w, src, what.c_str(), "ggrs_custom_kernel", w->layout_only ? nullptr : &c.mod, &c.fn);
    if (rc) return rc;
    ggrs_system_desc sd; memset(&sd, 0, sizeof sd);
    sd.kind = GGRS_SYS_CUSTOM; sd.comp[0] = (uint32_t)w->customs.size();
    sd.iparam[0] = d->iparam[0]; sd.iparam[1] = d->iparam[1];
    for (int k = 0; k < 4; ++k) sd.fparam[k] = d->fparam[k];
    w->customs.push_back(std::move(c));
    w->systems.push_back(sd);
    return GGRS_OK;
}
// THE PEER INDEX (include/ggrs_hip.h): registration only records; seal validates (host_seal.hpp peers_validate) and allocates the arrays next to the peer view.
int ggrs_hip_register_peer_index(ggrs_world* w, const ggrs_peer_index_desc* d) {
    if (!w) return GGRS_E_INVALID;
    if (!d) return w->fail(GGRS_E_INVALID, "register_peer_index without a desc");
    if (w->sealed) return w->fail(GGRS_E_INVALID, "register_peer_index after the world was sealed");
    if (w->peer_index.on) return w->fail(GGRS_E_INVALID, "register_peer_index: the world already has a peer index (over word %u of component %u, '%s'): one index per world in this version", w->peer_index.word, w->peer_index.comp, w->comps[w->peer_index.comp].name.c_str());
    if (d->comp >= w->comps.size() || d->word >= w->comps[d->comp].n_words) return w->fail(GGRS_E_INVALID, "register_peer_index names word %u of component %u, which is not registered", d->word, d->comp);
    if (d->flags) return w->fail(GGRS_E_INVALID, "register_peer_index over word %u of component %u ('%s'): unknown flags 0x%x", d->word, d->comp, w->comps[d->comp].name.c_str(), d->flags);
    if (d->n_buckets == 0 || d->n_buckets > GGRS_PEER_INDEX_MAX_BUCKETS)
        return w->fail(GGRS_E_INVALID, "register_peer_index over word %u of component %u ('%s'): n_buckets must be 1 .. %u (GGRS_PEER_INDEX_MAX_BUCKETS), not %u", d->word, d->comp, w->comps[d->comp].name.c_str(), GGRS_PEER_INDEX_MAX_BUCKETS, d->n_buckets);
    w->peer_index.on = true; w->peer_index.comp = d->comp; w->peer_index.word = d->word; w->peer_index.n_buckets = d->n_buckets;
    return GGRS_OK;
}
// DEVICE-RESIDENT ROLLBACK RESOURCES (include/ggrs_hip.h): init_resource + rollback_resource_with_copy, checksum_resource_with_hash, and the once-per-frame systems
// that mutate them.  Registration only records; seal validates the world (host_seal.hpp resources_validate) and puts the initial values into the live block.
int ggrs_hip_register_resource(ggrs_world* w, const char* name, uint32_t word_bytes, uint32_t n_words, const void* init_words, uint32_t* res_id_out) {
    if (!w || !name) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "register_resource '%s' after the world was sealed", name);
    if (w->resources.size() >= GGRS_RESOURCE_MAX) return w->fail(GGRS_E_INVALID, "resource '%s': at most %d resources per world (GGRS_RESOURCE_MAX)", name, GGRS_RESOURCE_MAX);
    if (word_bytes != 4 && word_bytes != 8) return w->fail(GGRS_E_INVALID, "resource '%s': word_bytes must be 4 or 8, not %u (1- and 2-byte words are not offered for resources)", name, word_bytes);
    if (n_words == 0 || n_words > GGRS_RESOURCE_MAX_BYTES / word_bytes || res_total_bytes(w) + word_bytes * n_words > GGRS_RESOURCE_MAX_BYTES)
        return w->fail(GGRS_E_INVALID, "resource '%s': %u words of %u bytes on top of %u bytes already registered: the resources of a world hold at most %d bytes together (GGRS_RESOURCE_MAX_BYTES)", name, n_words, word_bytes, res_total_bytes(w), GGRS_RESOURCE_MAX_BYTES);
    ggrs_world::Resource r; r.name = name; r.word_bytes = word_bytes; r.n_words = n_words;
    r.init.assign((size_t)word_bytes * n_words, 0);
    if (init_words) memcpy(r.init.data(), init_words, r.init.size());
    w->resources.push_back(std::move(r));
    res_layout(w);
    if (res_id_out) *res_id_out = (uint32_t)w->resources.size() - 1;
    return GGRS_OK;
}
int ggrs_hip_checksum_resource(ggrs_world* w, uint32_t res_id, const uint32_t* word_idx, uint32_t n_words) {
    if (!w) return GGRS_E_INVALID;
    if (res_id >= w->resources.size()) return w->fail(GGRS_E_INVALID, "checksum_resource: resource %u is not registered", res_id);
    ggrs_world::Resource& r = w->resources[res_id];
    if (w->sealed) return w->fail(GGRS_E_INVALID, "checksum_resource '%s' after the world was sealed", r.name.c_str());
    if (n_words && !word_idx) return w->fail(GGRS_E_INVALID, "checksum_resource '%s': word list is NULL", r.name.c_str());
    if (n_words > GGRS_MAX_CKS_UNITS) return w->fail(GGRS_E_INVALID, "checksum_resource '%s': checksum spec too long", r.name.c_str());
    for (uint32_t k = 0; k < n_words; ++k) if (word_idx[k] >= r.n_words) return w->fail(GGRS_E_INVALID, "checksum_resource '%s': word %u is not a word of the resource (%u words)", r.name.c_str(), word_idx[k], r.n_words);
    r.cks_words.assign(word_idx, word_idx + n_words);
    r.checksummed = true;
    return GGRS_OK;
}
int ggrs_hip_add_resource_system(ggrs_world* w, const ggrs_resource_system_desc* d) {
    if (!w || !d || !d->source) return GGRS_E_INVALID;
    const char* nm = d->name ? d->name : "resource_system";
    if (w->sealed) return w->fail(GGRS_E_INVALID, "add_resource_system '%s' after the world was sealed", nm);
    if (w->systems.size() >= GGRS_MAX_SYSTEMS) return w->fail(GGRS_E_INVALID, "resource system '%s': too many systems (GGRS_MAX_SYSTEMS)", nm);
    if (d->n_bindings == 0) return w->fail(GGRS_E_INVALID, "resource system '%s' has no binding: it could neither read nor change anything", nm);
    if (d->n_bindings > GGRS_RESOURCE_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "resource system '%s': at most %d bindings (GGRS_RESOURCE_MAX_BINDINGS), not %u", nm, GGRS_RESOURCE_MAX_BINDINGS, d->n_bindings);
    ggrs_world::ResSys rs; rs.name = nm; rs.source = d->source; rs.n_bind = d->n_bindings;
    for (uint32_t b = 0; b < rs.n_bind; ++b) {
        if (d->res[b] >= w->resources.size() || d->word[b] >= w->resources[d->res[b]].n_words)
            return w->fail(GGRS_E_INVALID, "resource system '%s': binding %u names word %u of resource %u, which is not registered", nm, b, d->word[b], d->res[b]);
        rs.res[b] = d->res[b]; rs.word[b] = d->word[b];
    }
    // a compile check against the system's own GgrsResources (a word it did not bind, or the other width, does not compile): the system itself only ever runs inside the generated kernel
    std::string src = GGRS_CUSTOM_ABI_TEXT;
    src += GGRS_FRAME_TEXT; src += GGRS_RESOURCES_TEXT; src += res_system_typedef(w, rs);
    src += "#line 1 \"ggrs_resource_system\"\n"; src += d->source;
    src += "\n#line 1 \"ggrs_resource_kernel\"\n"
           "extern \"C\" __global__ void ggrs_resource_kernel(GgrsCustomArgs a) {\n"
           "    GgrsFrame fr; fr.dt = a.fr.dt; fr.frame = a.fr.frame; fr.n_inputs = a.fr.n_inputs; fr.input_bytes = a.fr.input_bytes;\n"
           "    fr.input.p = a.fr.in; fr.input.ib = a.fr.input_bytes; fr.status = a.fr.in + a.fr.status_off;\n"
           "    for (int k = 0; k < 4; ++k) fr.fparam[k] = a.fr.fparam[k];\n"
           "    fr.iparam[0] = a.fr.iparam[0]; fr.iparam[1] = a.fr.iparam[1];\n"
           "    GgrsResources r; for (int k = 0; k < 8; ++k) r.w[k] = a.col_off[k];\n"
           "    ggrs_resource_system(r, fr);\n"
           "    for (int k = 0; k < 8; ++k) reinterpret_cast<ggrs_u64*>(a.state)[k] = r.w[k];\n"
           "}\n";
    DeviceGuard dg(w);
    const std::string what = "resource system '" + rs.name + "'";
    hipFunction_t fn = nullptr;
    const int rc = hiprtc_build(w, src, what.c_str(), "ggrs_resource_kernel", nullptr, &fn);
    if (rc) return rc;
    ggrs_system_desc sd; memset(&sd, 0, sizeof sd);
    sd.kind = GGRS_SYS_RESOURCE; sd.comp[0] = (uint32_t)w->res_systems.size();
    sd.iparam[0] = d->iparam[0]; sd.iparam[1] = d->iparam[1];
    for (int k = 0; k < 4; ++k) sd.fparam[k] = d->fparam[k];
    w->res_systems.push_back(std::move(rs));
    w->systems.push_back(sd);
    return GGRS_OK;
}
// RollbackApp::rollback_component_with_{copy,clone,reflect} are instances of  ComponentSnapshotPlugin<S: Strategy>  (snapshot/strategy.rs:22-40,
// component_snapshot.rs:42-63): S::Stored is what a snapshot holds.  Here: the Stored words and the HIP C++ of store / load.
int ggrs_hip_register_component_strategy(ggrs_world* w, uint32_t c, uint32_t stored_word_bytes, uint32_t stored_n_words, const char* source) {
    if (!w || c >= w->comps.size() || !source || !*source) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "register_component_strategy after the world was sealed");
    Comp& cc = w->comps[c];
    if (cc.no_rollback) return w->fail(GGRS_E_INVALID, "component %u is not registered for rollback: it has no snapshot strategy", c);
    if (stored_n_words == 0 || stored_n_words > GGRS_MAX_WORDS || (stored_word_bytes != 1 && stored_word_bytes != 2 && stored_word_bytes != 4 && stored_word_bytes != 8))
        return w->fail(GGRS_E_INVALID, "bad Stored shape (word bytes must be 1, 2, 4 or 8; 1..%d words)", GGRS_MAX_WORDS);
    cc.s_word_bytes = stored_word_bytes; cc.s_n_words = stored_n_words; cc.strat_source = source;
    return GGRS_OK;
}
// PlayerInputs<T>(Vec<(T::Input, InputStatus)>)  (src/lib.rs:98; inserted by AdvanceFrame, schedule_systems.rs:262-265)
int ggrs_hip_set_input_layout(ggrs_world* w, uint32_t input_bytes, uint32_t max_players) {
    if (!w) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "set_input_layout after the world was sealed");
    if (!w->systems.empty()) return w->fail(GGRS_E_INVALID, "set_input_layout must precede the first system of the schedule (custom systems are compiled against the layout when they are added)");
    if (input_bytes == 0 || input_bytes > GGRS_MAX_INPUT_BYTES || max_players == 0 || max_players > GGRS_MAX_PLAYERS)
        return w->fail(GGRS_E_INVALID, "input layout: 1..%d bytes per player, 1..%d players", GGRS_MAX_INPUT_BYTES, GGRS_MAX_PLAYERS);
    w->input_bytes = input_bytes; w->max_players = max_players;
    return GGRS_OK;
}
// A GgrsSchedule system that spawns Rollback entities (snapshot/rollback.rs:45-59; examples/stress_tests/particles.rs:258-270 is the built-in
// GGRS_SYS_PARTICLES_SPAWN): how many is the host's decision per AdvanceFrame (ggrs_request::spawn_count), what they are is the user's source.
int ggrs_hip_add_spawn_system(ggrs_world* w, const ggrs_spawn_system_desc* d) {
    if (!w || !d || !d->source) return GGRS_E_INVALID;
    if (w->sealed) return w->fail(GGRS_E_INVALID, "add_spawn_system after the world was sealed");
    if (w->systems.size() >= GGRS_MAX_SYSTEMS) return w->fail(GGRS_E_INVALID, "too many systems");
    for (auto& s : w->systems) if (s.kind == GGRS_SYS_SPAWN_CUSTOM || s.kind == GGRS_SYS_PARTICLES_SPAWN) return w->fail(GGRS_E_INVALID, "the schedule already holds a spawn system (one per world)");
    if (d->n_bindings > GGRS_CUSTOM_MAX_BINDINGS) return w->fail(GGRS_E_INVALID, "spawn system: at most %d bindings", GGRS_CUSTOM_MAX_BINDINGS);
    if (d->bundle_mask == 0 || (w->comps.size() < 64 && (d->bundle_mask >> w->comps.size()) != 0)) return w->fail(GGRS_E_INVALID, "spawn system: bundle_mask names no / unregistered components");
    ggrs_world::SpawnSys sp;
    sp.name = d->name ? d->name : "spawn"; sp.source = d->source; sp.n_bind = d->n_bindings; sp.bundle_mask = d->bundle_mask; sp.payload_stride = d->payload_stride;
    for (uint32_t c = 0; c < w->comps.size(); ++c) if (((sp.bundle_mask >> c) & 1ull) && w->comps[c].no_rollback)
        return w->fail(GGRS_E_INVALID, "spawn system '%s': component %u of the bundle is not registered for rollback", sp.name.c_str(), c);
    for (uint32_t i = 0; i < sp.n_bind; ++i) {
        if (d->comp[i] >= w->comps.size() || d->word[i] >= w->comps[d->comp[i]].n_words || !((sp.bundle_mask >> d->comp[i]) & 1ull))
            return w->fail(GGRS_E_INVALID, "spawn system '%s': binding %u names word %u of component %u, which is not a word of the bundle", sp.name.c_str(), i, d->word[i], d->comp[i]);
        sp.comp[i] = d->comp[i]; sp.word[i] = d->word[i];
    }
    ggrs_system_desc sd; memset(&sd, 0, sizeof sd);
    sd.kind = GGRS_SYS_SPAWN_CUSTOM; sd.comp[0] = (uint32_t)w->spawn_customs.size();
    sd.iparam[0] = d->iparam[0]; sd.iparam[1] = d->iparam[1];
    for (int k = 0; k < 4; ++k) sd.fparam[k] = d->fparam[k];
    w->spawn_customs.push_back(std::move(sp));
    w->systems.push_back(sd);
    return GGRS_OK;
}
// the file name a shipped code object of this source must carry (scripts/aot_build.py): NUL-terminated into buf
int ggrs_hip_aot_object_name(const char* source, char* buf, uint64_t cap) {
    if (!source || !buf || cap < 40) return GGRS_E_INVALID;
    const std::string n = jit_aot_name(source);
    memcpy(buf, n.c_str(), n.size() + 1);
    return GGRS_OK;
}
int ggrs_hip_generated_kernel_source(ggrs_world* w, uint32_t form, char* buf, uint64_t cap, uint64_t* needed, int compile) {
    if (!w || (form != GGRS_KERNEL_FORM_TILES && form != GGRS_KERNEL_FORM_STEADY)) return GGRS_E_INVALID;
    if (!w->sealed) {
        if (!w->layout_only) { DeviceGuard dg(w); const int rc = seal(w); if (rc) return rc; }
        else { build_layout(w); const int prc = peers_validate(w); if (prc) return prc; const int frc = effects_validate(w); if (frc) return frc; const int crc = commands_validate(w); if (crc) return crc; const int rrc = resources_validate(w); if (rrc) return rrc; const int drc = reduces_validate(w); if (drc) return drc; const int xrc = remote_validate(w); if (xrc) return xrc; const int vrc = values_validate(w); if (vrc) return vrc; const int src_ = sums_validate(w); if (src_) return src_; }   // host arithmetic only: offsets of every mask and column; the peer-, effect-, command-, resource, reduce, remote, value and sum rules
    }
    std::string src;
    if (!jit_source(w, src)) return w->fail(GGRS_E_INVALID, "the kernel generator does not cover this world (a system writes a live-only component, or more than %u four-byte units / %u words per entity)", JIT_MAX_UNITS, JIT_MAX_COLS);
    if (form == GGRS_KERNEL_FORM_STEADY) {
        src = jit_specialise(src, jit_steady_sig(w));
        if (src.empty()) return w->fail(GGRS_E_INVALID, "the generated kernel's text could not be specialised");
    }
    if (needed) *needed = src.size() + 1;
    if (buf && cap) { const uint64_t n = std::min<uint64_t>(cap, src.size() + 1); memcpy(buf, src.c_str(), n); buf[n - 1] = 0; }
    if (compile) { hipFunction_t fn = nullptr; return hiprtc_build(w, src, "generated request-group kernel", "ggrs_jit_tick", nullptr, &fn); }
    return GGRS_OK;
}
// Test hook (no ggrs_hip_ prefix, not in the header): the text of the checksum-parts kernel generated for a world with a user-written hasher (kernel_gen.hpp
// jit_parts_source; any world gets a text); compile != 0: also built for gfx950 with hiprtc.  Works on a GGRS_WORLD_LAYOUT_ONLY world, as the call above
int ggrs_dbg_parts_kernel_source(ggrs_world* w, char* buf, uint64_t cap, uint64_t* needed, int compile) {
    if (!w) return GGRS_E_INVALID;
    if (!w->sealed) {
        if (!w->layout_only) { DeviceGuard dg(w); const int rc = seal(w); if (rc) return rc; }
        else build_layout(w);
    }
    const std::string src = jit_parts_source(w);
    if (needed) *needed = src.size() + 1;
    if (buf && cap) { const uint64_t n = std::min<uint64_t>(cap, src.size() + 1); memcpy(buf, src.c_str(), n); buf[n - 1] = 0; }
    if (compile) { hipFunction_t fn = nullptr; return hiprtc_build(w, src, "generated checksum-parts kernel", "ggrs_jit_parts", nullptr, &fn); }
    return GGRS_OK;
}
// Test hook (not part of the C ABI: no ggrs_hip_ prefix, not in include/ggrs_hip.h): the specialiser's token rule on arbitrary text --
// tests/test_generated_kernel.py feeds it identifiers no generator emits yet.  Returns the number of replacements, -1 when `out` is too small.
int ggrs_dbg_replace_token(const char* body, const char* tok, const char* val, char* out, uint64_t cap) {
    if (!body || !tok || !val || !out || !*tok) return -1;
    std::string b = body;
    const uint32_t n = jit_replace_token(b, tok, val);
    if (b.size() + 1 > cap) return -1;
    memcpy(out, b.c_str(), b.size() + 1);
    return (int)n;
}
// Test hooks (no ggrs_hip_ prefix, not in the header; neither changes a result):
//   ggrs_dbg_set_lazy_live     0 = every tick writes the live block (the A/B of profiles/r05h), 2 = every eligible list leaves it unwritten whatever its size and
//                              streak (the fuzzer: tests/test_fuzz_requests.py), 1 = the default policy
//   ggrs_dbg_set_spec_shapes   places in the table of group shapes / specialised kernels (default 16), so that a P2P session's eight rollback lengths
//                              exercise the least-recently-used eviction (tests/test_gpu_gen_groups.py)
//   ggrs_dbg_set_spec_resident 0 = a device-spawn world's resident form is told that the device does NOT hold its grid of any specialised copy (host_groups.hpp
//                              jit_spec_fits), so the general kernel goes on running and kernel_info lists the copies under "failed"; -1 = the device is asked
//   ggrs_dbg_set_value_tags    0 = no Save skips a column on its value tags, 1 = every world does, -1 = by size (the default: host_world.hpp VTAGS_MIN_BYTES);
//                              before the world is sealed
int ggrs_dbg_set_value_tags(ggrs_world* w, int mode) { if (!w || w->sealed) return -1; w->vtags_mode = mode; return 0; }
int ggrs_dbg_set_lazy_live(ggrs_world* w, int on) { if (!w) return -1; w->lazy_live_on = on; return 0; }
//   ggrs_dbg_set_reduce_stripes  lines of the reduce inbox (1..64, default RD_STRIPES = 64), before seal: what scripts/bench_reduces.py varies
//   ggrs_dbg_reduce_inbox      the bytes of the reduce inbox (stripes x 64) after everything queued on the world's stream has run: returns how many bytes the inbox has
//                              (min(cap, that) are copied), -1 for a world without one -- it must hold identities whenever a host call returns
int ggrs_dbg_set_reduce_stripes(ggrs_world* w, int n) { if (!w || w->sealed || n < 1 || n > 64) return -1; w->rd_stripes = (uint32_t)n; return 0; }
int64_t ggrs_dbg_reduce_inbox(ggrs_world* w, void* out, uint64_t cap) {
    if (!w || !w->rd_inbox.d) return -1;
    DeviceGuard dg(w);
    const uint64_t bytes = (uint64_t)w->rd_inbox.stripes * 64u;
    if (hipMemcpyAsync(out, w->rd_inbox.d, std::min(cap, bytes), hipMemcpyDeviceToHost, w->stream) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) return -1;
    return (int64_t)bytes;
}
//   ggrs_dbg_remote_inbox      the words of the remote inbox (one u32 per slot of the padded capacity) after everything queued on the world's stream has run: returns
//                              how many bytes the inbox has (min(cap, that) are copied), -1 for a world without one -- it must hold zeros whenever a host call returns
int64_t ggrs_dbg_remote_inbox(ggrs_world* w, void* out, uint64_t cap) {
    if (!w || !w->rx_inbox.d) return -1;
    DeviceGuard dg(w);
    const uint64_t bytes = w->cap_pad * 4u;
    if (hipMemcpyAsync(out, w->rx_inbox.d, std::min(cap, bytes), hipMemcpyDeviceToHost, w->stream) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) return -1;
    return (int64_t)bytes;
}
//   ggrs_dbg_sum_partials      the sum partials of summed word `word` (8 bytes per 64-slot unit: a float in the low four bytes, or a double) after everything queued on the
//                              world's stream has run: returns how many bytes the word's array has (min(cap, that) are copied), -1 for a world without one or a word it does
//                              not have.  Only the entries of the units the last launch covered mean anything
int64_t ggrs_dbg_sum_partials(ggrs_world* w, uint32_t word, void* out, uint64_t cap) {
    if (!w || !w->sum_part.d || word >= w->sum_part.n_words) return -1;
    DeviceGuard dg(w);
    const uint64_t bytes = (uint64_t)w->sum_part.units * 8u;
    if (hipMemcpyAsync(out, w->sum_part.d + (uint64_t)word * bytes, std::min(cap, bytes), hipMemcpyDeviceToHost, w->stream) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) return -1;
    return (int64_t)bytes;
}
//   ggrs_dbg_value_winners     the winner words of value-bound component `comp` (one u64 per slot of the padded capacity) after everything queued on the world's stream
//                              has run: returns how many bytes they have (min(cap, that) are copied), -1 for a world without value bindings or a component no value
//                              binding names -- they must hold zeros whenever a host call returns
int64_t ggrs_dbg_value_winners(ggrs_world* w, uint32_t comp, void* out, uint64_t cap) {
    if (!w || !w->has_values || !w->rv_inbox.alloc) return -1;
    const uint64_t* d = nullptr;
    for (uint32_t k = 0; k < w->rx_inbox.n_comps; ++k) if (w->rx_inbox.comp[k] == comp) d = w->rv_inbox.d_win[k];
    if (!d) return -1;
    DeviceGuard dg(w);
    const uint64_t bytes = w->cap_pad * 8u;
    if (hipMemcpyAsync(out, d, std::min(cap, bytes), hipMemcpyDeviceToHost, w->stream) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) return -1;
    return (int64_t)bytes;
}
int ggrs_dbg_set_spec_resident(ggrs_world* w, int mode) { if (!w || (mode != -1 && mode != 0)) return -1; w->spec_resident = mode; return 0; }
int ggrs_dbg_set_spec_shapes(ggrs_world* w, int n) { if (!w || n < 1 || n > 64) return -1; w->spec_shapes = n; return 0; }
int ggrs_hip_set_frame_rate(ggrs_world* w, uint64_t fps) { if (!w || fps == 0) return GGRS_E_INVALID; w->fps = fps; return GGRS_OK; }

// entry points that read or edit the live block's BYTES: a lazily skipped live block (host_groups.hpp) is materialised first; a world whose systems spawn
// on the device learns its RollbackOrdered::len from the last launch (len_sync)
static int seal_live(ggrs_world* w) { int rc = seal(w); if (rc) return rc; rc = len_sync(w); if (rc) return rc; return materialise_live(w); }

int ggrs_hip_spawn(ggrs_world* w, uint64_t count, uint64_t comp_mask, const void* const* cols, uint64_t* first_slot) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (!range_ok(w->len, count, w->capacity)) return w->fail(GGRS_E_CAPACITY, "spawn of %llu exceeds capacity %llu", (unsigned long long)count, (unsigned long long)w->capacity);
    const uint64_t first = w->len;
    if (first_slot) *first_slot = first;
    if (count == 0) return GGRS_OK;
    uint32_t ci = 0;
    for (uint32_t c = 0; c < w->comps.size(); ++c) {
        if (!((comp_mask >> c) & 1ULL)) continue;
        const Comp& cc = w->comps[c];
        bool any_null = false;
        for (uint32_t k = 0; k < cc.n_words; ++k) if (!cols || !cols[ci + k]) any_null = true;
        if (any_null) { rc = fill_defaults(w, c, first, count); if (rc) return rc; }
        for (uint32_t k = 0; k < cc.n_words; ++k) {
            const void* src = cols ? cols[ci + k] : nullptr;
            if (src) { rc = copy_column(w, cc.col_base + k, first, count, const_cast<void*>(src), true); if (rc) return rc; }
        }
        ver_touch_comp(w, c); live_tags_lost_comp(w, c);            // new rows in every column of the bundle
        ci += cc.n_words;
    }
    ver_sync_live(w);
    rc = set_masks_for_range(w, first, count, comp_mask); if (rc) return rc;
    w->len += count;
    w->live.dirty_len = std::max(w->live.dirty_len, w->len);
    if (w->dev_spawn) { const uint64_t l = w->len; HIPCHK(w, hipMemcpyAsync(w->live.ptr, &l, 8, hipMemcpyHostToDevice, w->stream)); }   // the kernels read RollbackOrdered::len from the block's header
    w->pending_valid = false;
    HIPCHK(w, hipStreamSynchronize(w->stream));     // host buffers may be freed on return
    return GGRS_OK;
}
int ggrs_hip_despawn(ggrs_world* w, uint64_t slot) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (slot >= w->len) return w->fail(GGRS_E_INVALID, "slot out of range");
    hipLaunchKernelGGL(k_edit_mask_bit, dim3(1), dim3(1), 0, w->stream, w->live.ptr, w->off_alive, slot, 0);
    HIPCHK(w, hipGetLastError());
    w->pending_valid = false;
    return GGRS_OK;
}
int ggrs_hip_despawn_rollback(ggrs_world* w, uint64_t slot) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (slot >= w->len) return w->fail(GGRS_E_INVALID, "slot out of range");
    if (w->confirmed < w->frame) {                 // despawn.rs:129-137: insert RollbackDespawned(frame)
        w->marks_possible = true;
        hipLaunchKernelGGL(k_mark_despawned, dim3(1), dim3(1), 0, w->stream, w->live.ptr, w->off_alive, w->marks, slot, w->frame);
    } else {                                       // despawn.rs:140-142: frame already confirmed -> plain despawn
        hipLaunchKernelGGL(k_edit_mask_bit, dim3(1), dim3(1), 0, w->stream, w->live.ptr, w->off_alive, slot, 0);
    }
    HIPCHK(w, hipGetLastError());
    w->pending_valid = false;
    return GGRS_OK;
}
int ggrs_hip_insert_component(ggrs_world* w, uint32_t c, uint64_t slot, const void* words) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size() || slot >= w->len || !words) return w->fail(GGRS_E_INVALID, "bad insert_component arguments");
    const Comp& cc = w->comps[c];
    for (uint32_t k = 0; k < cc.n_words; ++k)
        { rc = copy_column(w, cc.col_base + k, slot, 1, const_cast<uint8_t*>((const uint8_t*)words + (size_t)k * cc.word_bytes), true); if (rc) return rc; }
    ver_touch_comp(w, c); live_tags_lost_comp(w, c); ver_sync_live(w);
    hipLaunchKernelGGL(k_edit_mask_bit, dim3(1), dim3(1), 0, w->stream, w->live.ptr, w->off_present[c], slot, 1);
    HIPCHK(w, hipGetLastError());
    w->pending_valid = false;
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}
int ggrs_hip_remove_component(ggrs_world* w, uint32_t c, uint64_t slot) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size() || slot >= w->len) return w->fail(GGRS_E_INVALID, "bad remove_component arguments");
    hipLaunchKernelGGL(k_edit_mask_bit, dim3(1), dim3(1), 0, w->stream, w->live.ptr, w->off_present[c], slot, 0);
    HIPCHK(w, hipGetLastError());
    ver_touch(w, ver_presence(w, c)); ver_sync_live(w);           // the presence mask changed, the columns did not
    w->pending_valid = false;
    return GGRS_OK;
}
int ggrs_hip_upload_word(ggrs_world* w, uint32_t c, uint32_t word, uint64_t first, uint64_t count, const void* src) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size() || word >= w->comps[c].n_words || !range_ok(first, count, w->capacity) || !src) return w->fail(GGRS_E_INVALID, "bad upload_word arguments");
    const Comp& cc = w->comps[c];
    rc = copy_column(w, cc.col_base + word, first, count, const_cast<void*>(src), true); if (rc) return rc;
    ver_touch(w, cc.col_base + word); live_tags_lost(w, cc.col_base + word); ver_sync_live(w);
    HIPCHK(w, hipStreamSynchronize(w->stream));
    w->pending_valid = false;
    return GGRS_OK;
}
int ggrs_hip_download_word(ggrs_world* w, uint32_t c, uint32_t word, uint64_t first, uint64_t count, void* dst) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size() || word >= w->comps[c].n_words || !range_ok(first, count, w->capacity) || !dst) return w->fail(GGRS_E_INVALID, "bad download_word arguments");
    const Comp& cc = w->comps[c];
    rc = copy_column(w, cc.col_base + word, first, count, dst, false); if (rc) return rc;
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}
// world.resource::<R>() / world.resource_mut::<R>() of a device resource: the live block's current cell.  As for the column traffic above a lazily skipped live block is
// materialised first (seal_live) and the copy is ordered on the world's stream; a write also ends the lazy-live streak -- the next list may read what was written.
int ggrs_hip_resource_read(ggrs_world* w, uint32_t res_id, void* words_out) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (res_id >= w->resources.size() || !words_out) return w->fail(GGRS_E_INVALID, "bad resource_read arguments (resource %u of %zu)", res_id, w->resources.size());
    const ggrs_world::Resource& r = w->resources[res_id];
    HIPCHK(w, hipMemcpyAsync(words_out, w->live.ptr + RES_CELL_OFF + w->live.res_cell * RES_CELL_BYTES + r.off, (size_t)r.word_bytes * r.n_words, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}
int ggrs_hip_resource_write(ggrs_world* w, uint32_t res_id, const void* words) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (res_id >= w->resources.size() || !words) return w->fail(GGRS_E_INVALID, "bad resource_write arguments (resource %u of %zu)", res_id, w->resources.size());
    const ggrs_world::Resource& r = w->resources[res_id];
    HIPCHK(w, hipMemcpyAsync(w->live.ptr + RES_CELL_OFF + w->live.res_cell * RES_CELL_BYTES + r.off, words, (size_t)r.word_bytes * r.n_words, hipMemcpyHostToDevice, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));                        // (the caller's buffer is free again when the call returns)
    w->load_open_streak = 0; w->pending_valid = false;
    return GGRS_OK;
}
static int download_mask(ggrs_world* w, uint64_t off, uint64_t* dst, uint64_t n) {
    const uint64_t have = w->cap_pad / 64;
    const uint64_t m = n < have ? n : have;
    HIPCHK(w, hipMemcpyAsync(dst, w->live.ptr + off, m * 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    for (uint64_t k = m; k < n; ++k) dst[k] = 0;
    return GGRS_OK;
}
int ggrs_hip_download_alive(ggrs_world* w, uint64_t* dst, uint64_t n) {
    if (!w || !dst) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    return download_mask(w, w->off_alive, dst, n);
}
int ggrs_hip_download_present(ggrs_world* w, uint32_t c, uint64_t* dst, uint64_t n) {
    if (!w || !dst) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size()) return w->fail(GGRS_E_INVALID, "bad component");
    rc = download_mask(w, w->off_present[c], dst, n); if (rc) return rc;
    if (w->comps[c].no_rollback && n) {
        // a non-rollback component dies with its entity: it exists while the entity is alive or
        // disabled (its live-only presence bit is cleaned lazily, when the slot is re-created)
        std::vector<uint64_t> a(n), d(n);
        rc = download_mask(w, w->off_alive, a.data(), n); if (rc) return rc;
        rc = download_mask(w, w->marks.off_disabled, d.data(), n); if (rc) return rc;
        for (uint64_t k = 0; k < n; ++k) dst[k] &= (a[k] | d[k]);
    }
    return GGRS_OK;
}
int ggrs_hip_download_disabled(ggrs_world* w, uint64_t* dst, uint64_t n) {
    if (!w || !dst) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    return download_mask(w, w->marks.off_disabled, dst, n);
}
int ggrs_hip_download_despawned_frames(ggrs_world* w, uint64_t first, uint64_t count, int32_t* frames) {
    if (!w || !frames) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (!range_ok(first, count, w->capacity)) return w->fail(GGRS_E_INVALID, "bad download_despawned_frames range");
    if (count) HIPCHK(w, hipMemcpyAsync(frames, w->live.ptr + w->marks.off_dframe + first * 4, (size_t)count * 4, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}
int ggrs_hip_column_device_ptr(ggrs_world* w, uint32_t c, uint32_t word, void** p, uint64_t* tile_stride) {
    if (!w || !p) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    if (c >= w->comps.size() || word >= w->comps[c].n_words) return w->fail(GGRS_E_INVALID, "bad column");
    *p = w->live.ptr + w->col_off[w->comps[c].col_base + word];
    w->col_ext[w->comps[c].col_base + word] = 1;                   // whoever holds this pointer may write the column at any time: no row-version shortcuts for it
    if (tile_stride) *tile_stride = w->col_ts[w->comps[c].col_base + word];
    return GGRS_OK;
}
uint64_t ggrs_hip_len(ggrs_world* w) { if (!w) return 0; if (w->len_stale) { DeviceGuard dg(w); (void)len_sync(w); } return w->len; }
int ggrs_hip_active_count(ggrs_world* w, uint64_t* out) {
    if (!w || !out) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    const uint64_t n = (w->live.dirty_len + 63) / 64;
    std::vector<uint64_t> m(n ? n : 1, 0);
    if (n) { rc = download_mask(w, w->off_alive, m.data(), n); if (rc) return rc; }
    uint64_t a = 0; for (uint64_t k = 0; k < n; ++k) a += (uint64_t)__builtin_popcountll(m[k]);
    *out = a;
    return GGRS_OK;
}

int32_t ggrs_hip_frame(ggrs_world* w) { return w ? w->frame : 0; }
int ggrs_hip_set_frame(ggrs_world* w, int32_t f) { if (!w) return GGRS_E_INVALID; w->frame = f; return GGRS_OK; }
int ggrs_hip_set_depth(ggrs_world* w, uint32_t d) {
    if (!w) return GGRS_E_INVALID;
    if (d > w->max_depth) return w->fail(GGRS_E_INVALID, "depth %u exceeds provisioned max_depth %u", d, w->max_depth);
    w->depth = d;
    return GGRS_OK;
}
int ggrs_hip_set_confirmed(ggrs_world* w, int has, int32_t f) { if (!w) return GGRS_E_INVALID; w->has_confirmed = has != 0; w->confirmed = f; return GGRS_OK; }
int ggrs_hip_has_snapshot(ggrs_world* w, int32_t f) {
    if (!w) return 0;
    for (int32_t x : w->ring_frame) if (x == f) return 1;
    return 0;
}
uint64_t ggrs_hip_snapshot_count(ggrs_world* w) { return w ? w->ring_frame.size() : 0; }
int ggrs_hip_set_synctest_check_distance(ggrs_world* w, int32_t cd) { if (!w) return GGRS_E_INVALID; w->synctest_cd = cd; return GGRS_OK; }

int ggrs_hip_save(ggrs_world* w, uint64_t out[2]) {
    if (!w) return GGRS_E_INVALID;
    if (!w->pending.empty()) return w->fail(GGRS_E_INVALID, "synchronous request while %zu enqueued batches are uncollected", w->pending.size());
    DeviceGuard dg(w);
    int rc = seal(w); if (rc) return rc;
    if (GroupRunner run = group_runner(w)) { ggrs_request r; memset(&r, 0, sizeof r); r.kind = GGRS_REQ_SAVE; r.frame = w->frame; return run(w, &r, 1, out, 0, true, nullptr); }
    rc = do_save(w, 0); if (rc) return rc;
    return read_back(w, 1, out);
}
int ggrs_hip_load(ggrs_world* w, int32_t frame) {
    if (!w) return GGRS_E_INVALID;
    if (!w->pending.empty()) return w->fail(GGRS_E_INVALID, "synchronous request while %zu enqueued batches are uncollected", w->pending.size());
    DeviceGuard dg(w);
    int rc = seal(w); if (rc) return rc;
    if (GroupRunner run = group_runner(w)) { ggrs_request r; memset(&r, 0, sizeof r); r.kind = GGRS_REQ_LOAD; r.frame = frame; return run(w, &r, 1, nullptr, 0, true, nullptr); }
    return do_load(w, frame);
}
int ggrs_hip_advance(ggrs_world* w, uint32_t dt_bits, const uint8_t* inputs, uint32_t n_inputs,
                     uint64_t spawn_count, const float* vx, const float* vy) {
    if (!w) return GGRS_E_INVALID;
    if (!w->pending.empty()) return w->fail(GGRS_E_INVALID, "synchronous request while %zu enqueued batches are uncollected", w->pending.size());
    DeviceGuard dg(w);
    int rc = seal(w); if (rc) return rc;
    ggrs_request r; memset(&r, 0, sizeof r);
    r.kind = GGRS_REQ_ADVANCE; r.dt_bits = dt_bits; r.inputs = inputs; r.n_inputs = n_inputs;
    r.spawn_count = spawn_count; r.spawn_vx = vx; r.spawn_vy = vy;
    rc = validate_requests(w, &r, 1); if (rc) return rc;
    if (GroupRunner run = group_runner(w)) return run(w, &r, 1, nullptr, 0, true, nullptr);
    return do_advance(w, r);
}

int ggrs_hip_handle_requests(ggrs_world* w, const ggrs_request* reqs, uint32_t n, uint64_t* checksums_out) {
    if (!w || (!reqs && n)) return GGRS_E_INVALID;
    TraceRange tr("HandleRequests");
    DeviceGuard dg(w);
    int rc = seal(w); if (rc) return rc;
    if (!w->pending.empty()) return w->fail(GGRS_E_INVALID, "handle_requests while %zu enqueued batches are uncollected", w->pending.size());
    rc = validate_requests(w, reqs, n); if (rc) return rc;
    if (GroupRunner run = group_runner(w)) {
        rc = run(w, reqs, n, checksums_out, 0, true, nullptr);
        if (rc && w->stream) { (void)hipStreamSynchronize(w->stream); w->folds.clear(); w->rows_used = 0; w->rows_tail = 0; }   // (nothing is pending in the synchronous API)
        return rc;
    }
    uint32_t ns = 0;
    for (uint32_t i = 0; i < n && rc == GGRS_OK; ++i) {
        const ggrs_request& r = reqs[i];
        trace_request(w, r);
        apply_synctest_confirmed(w);
        switch (r.kind) {
        case GGRS_REQ_SAVE:
            if (ns >= w->max_results) {                   // flush a full result page
                rc = read_back(w, ns, checksums_out); if (rc) break;
                checksums_out += 2 * (uint64_t)ns; ns = 0;
            }
            rc = do_save(w, ns); ++ns; break;
        case GGRS_REQ_LOAD: rc = do_load(w, r.frame); break;
        case GGRS_REQ_ADVANCE: rc = do_advance(w, r); break;
        default: rc = w->fail(GGRS_E_INVALID, "unknown request kind %u", r.kind);
        }
    }
    if (rc) { if (w->stream) (void)hipStreamSynchronize(w->stream); return rc; }
    return read_back(w, ns, checksums_out);
}
// Asynchronous pair: the request list is only ENQUEUED on the world's stream (all host-side bookkeeping --
// frame counters, ring push/confirm/rollback -- happens now, in request order); the Checksum(u128)s are
// fetched later, oldest batch first.  ggrs reads a SaveGameState cell no earlier than the next
// advance_frame(), so a host shim collects right before that call and the GPU tick overlaps the rest of
// the host's frame instead of blocking it.
// bs != nullptr: a branch step (ggrs_hip_fanout_step_branches) -- `reqs` is its prefix, the branches' launch and Checksum(u128)s follow in the same batch
static int enqueue_impl(ggrs_world* w, const ggrs_request* reqs, uint32_t n, const ggrs_branch_step* bs, BranchKeep* keep, uint32_t* n_saves_out) {
    if (!w || (!reqs && n)) return GGRS_E_INVALID;
    TraceRange tr("HandleRequests");
    DeviceGuard dg(w);
    int rc = seal(w); if (rc) return rc;
    const double t_in = w->tl.on ? tl_now_us() : 0;
    rc = validate_requests(w, reqs, n); if (rc) return rc;
    if (bs) { rc = validate_branch_step(w, *bs); if (rc) return rc; }
    if (w->tl.on) w->tl.validate_us += tl_now_us() - t_in;
    uint32_t n_save = 0;
    for (uint32_t i = 0; i < n; ++i) n_save += reqs[i].kind == GGRS_REQ_SAVE;
    const uint32_t n_save_prefix = n_save;
    if (bs) n_save += bs->n_branches * ((bs->flags & GGRS_BRANCH_SAVE_LAST) ? bs->n_frames : bs->n_frames - 1);
    if (n_save > w->max_results / 4 || w->pending_results + n_save > w->max_results / 2 || w->pending.size() >= 16)
        return w->fail(GGRS_E_INVALID, "too many uncollected checksums (%u pending + %u new): call ggrs_hip_collect_checksums", w->pending_results, n_save);
    ggrs_world::PendingBatch b;
    b.first = (w->res_head + n_save > w->max_results) ? 0u : w->res_head;
    b.count = n_save;
    const size_t folds_before = w->folds.size();
    const uint64_t ff_id0 = w->ff_next_id;
    if (w->event_pool.empty()) { hipEvent_t e; HIPCHK(w, hipEventCreateWithFlags(&e, hipEventDisableTiming)); w->event_pool.push_back(e); }
    b.ev = w->event_pool.back(); w->event_pool.pop_back();
    w->batch_ev_attached = false;
    if (w->dev_results_dst) w->dev_results_first = b.first;          // the consumer's device copy starts with this batch's first Checksum(u128)
    if (GroupRunner run = group_runner(w)) {
        w->batch_ev = b.ev;
        rc = run(w, reqs, n, nullptr, b.first, false, nullptr);
        if (rc == GGRS_OK && bs) rc = run_branch_step(w, *bs, b.first + n_save_prefix, keep);
        // a component under a Strategy: the live world the prefix left holds the component itself, the list form's closing LoadGameState(F) leaves load(store(x)),
        // which a lossy Stored form makes another value -- the step ends with that LoadWorld (every other world: the two are the same bytes, nothing runs)
        if (rc == GGRS_OK && bs && w->has_strategy) {
            ggrs_request ld; memset(&ld, 0, sizeof ld); ld.kind = GGRS_REQ_LOAD; ld.frame = w->frame;
            rc = run(w, &ld, 1, nullptr, b.first, false, nullptr);
        }
        w->batch_ev = nullptr;
        if (rc) {
            w->event_pool.push_back(b.ev); (void)hipStreamSynchronize(w->stream);
            while (w->folds.size() > folds_before) w->folds.pop_back();
            if (w->ff_pending.valid && w->ff_pending.id >= ff_id0) w->ff_pending.valid = false;      // its HostFold is gone with the failed list
            return rc;
        }
    } else {
        // worlds without request-group kernels: one launch per request, enqueued like the groups are; every
        // Save's fold writes straight into its slot of the pinned result ring, nothing is waited for here
        uint32_t ns = 0;
        for (uint32_t i = 0; i < n && rc == GGRS_OK; ++i) {
            const ggrs_request& r = reqs[i];
            trace_request(w, r);
            apply_synctest_confirmed(w);
            switch (r.kind) {
            case GGRS_REQ_SAVE: rc = do_save(w, b.first + ns); ++ns; break;
            case GGRS_REQ_LOAD: rc = do_load(w, r.frame); break;
            case GGRS_REQ_ADVANCE: rc = do_advance(w, r); break;
            default: rc = w->fail(GGRS_E_INVALID, "unknown request kind %u", r.kind);
            }
        }
        if (rc) { (void)hipStreamSynchronize(w->stream); return rc; }
    }
    if (!w->batch_ev_attached) HIPCHK(w, hipEventRecord(b.ev, w->stream));      // (else the event rides on the list's last kernel)
    w->res_head = b.first + n_save; w->pending_results += n_save;
    b.n_folds = (uint32_t)(w->folds.size() - folds_before);
    b.stage_end = w->stage_used;
    if (n_saves_out) *n_saves_out = n_save;
    w->pending.push_back(std::move(b));
    if (w->tl.on) { w->tl.enqueue_us += tl_now_us() - t_in; ++w->tl.n_enqueue; }
    return GGRS_OK;
}
int ggrs_hip_enqueue_requests(ggrs_world* w, const ggrs_request* reqs, uint32_t n, uint32_t* n_saves_out) { return enqueue_impl(w, reqs, n, nullptr, nullptr, n_saves_out); }
// the batch's event, waited for by polling (hipEventQuery returns in 0.06 us; hipEventSynchronize on an event that is NOT complete yet costs
// 0.7 us more per tick of a 5.6 us kernel: scripts/ubench_launch, profiles/r05a) for up to GGRS_SPIN_WAIT_US, then by the runtime's wait
static int wait_batch_event(ggrs_world* w, hipEvent_t ev) {
    if (w->knobs.spin_wait_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 1; ; ++it) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return GGRS_OK;
            if (e != hipErrorNotReady) { (void)hipGetLastError(); break; }
            if ((it & 31u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(w->knobs.spin_wait_us)) break;
            cpu_relax();
        }
        (void)hipGetLastError();                                     // (hipErrorNotReady is sticky in hipGetLastError)
    }
    HIPCHK(w, hipEventSynchronize(ev));
    return GGRS_OK;
}
int ggrs_hip_collect_checksums(ggrs_world* w, uint64_t* checksums_out, uint32_t max_saves, uint32_t* n_saves_out) {
    if (!w) return GGRS_E_INVALID;
    if (w->pending.empty()) return w->fail(GGRS_E_INVALID, "no enqueued batch to collect");
    DeviceGuard dg(w);
    ggrs_world::PendingBatch& b = w->pending.front();
    if (b.count > max_saves || (b.count && !checksums_out)) return w->fail(GGRS_E_INVALID, "oldest batch holds %u checksums, room for %u", b.count, max_saves);
    const double t_in = w->tl.on ? tl_now_us() : 0;
    // a fold-forward group whose rows nothing took along yet: queue k_ff_fold BEFORE waiting (it runs right behind the batch's kernel)
    if (w->ff_pending.valid) for (uint32_t k = 0; k < b.n_folds && k < w->folds.size(); ++k) if (w->folds[k].ff_id == w->ff_pending.id) { int rc = ff_flush(w); if (rc) return rc; break; }
    int rc = wait_batch_event(w, b.ev); if (rc) return rc;
    if (w->tl.on) w->tl.wait_us += tl_now_us() - t_in;
    rc = run_host_folds(w, b.n_folds); if (rc) return rc;
    if (b.count) {
        if (!b.host.empty()) memcpy(checksums_out, b.host.data(), (size_t)b.count * 16);
        else memcpy(checksums_out, w->h_results + 2 * (size_t)b.first, (size_t)b.count * 16);
    }
    if (n_saves_out) *n_saves_out = b.count;
    w->pending_results -= b.count;
    w->event_pool.push_back(b.ev);
    const uint64_t stage_end = b.stage_end;
    w->pending.pop_front();
    // the batch's launches are done: its spawn payloads (and everything staged before them) are free again
    if (w->pending.empty()) stage_ring_reset(w); else if (stage_end) w->stage_tail = stage_end;
    // Nothing is queued behind this batch and its results were seen through pinned memory: the runtime itself has not looked at the stream yet.  One
    // non-blocking query lets it retire the finished commands now, so that a device-wide synchronise that follows finds an idle stream
    if (w->pending.empty() && !w->prof) { (void)hipStreamQuery(w->stream); (void)hipGetLastError(); }
    if (w->tl.on) { w->tl.collect_us += tl_now_us() - t_in; ++w->tl.n_collect; }
    return GGRS_OK;
}
// Where the HOST spends a tick.  enable: 1 = reset and start, 0 = stop, -1 = leave as is.  us_out[GGRS_TIMELINE_FIELDS] = microseconds
// summed since the start: {enqueue call, of it: validation, of it: launch calls (hipModuleLaunchKernel / hipExtModuleLaunchKernel), collect call, of it: the
// batch event, of it: fold-forward tags, of it: hashing / folding on the host}; counts_out[3] = {enqueue calls, collect calls, launches}.
int ggrs_hip_host_timeline(ggrs_world* w, int enable, double* us_out, uint64_t* counts_out) {
    if (!w) return GGRS_E_INVALID;
    if (us_out) { const HostTimeline& t = w->tl; const double v[GGRS_TIMELINE_FIELDS] = {t.enqueue_us, t.validate_us, t.launch_us, t.collect_us, t.wait_us, t.tag_wait_us, t.fold_us}; memcpy(us_out, v, sizeof v); }
    if (counts_out) { counts_out[0] = w->tl.n_enqueue; counts_out[1] = w->tl.n_collect; counts_out[2] = w->tl.n_launches; }
    if (enable == 1) { w->tl = HostTimeline{}; w->tl.on = true; }
    else if (enable == 0) w->tl.on = false;
    return GGRS_OK;
}
uint32_t ggrs_hip_pending_batches(ggrs_world* w) { return w ? (uint32_t)w->pending.size() : 0; }

int ggrs_hip_synchronize(ggrs_world* w) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    if (w->sealed) { const int rc = ff_flush(w); if (rc) return rc; }          // rows a fold-forward launch left behind: nothing may be left half-done on the stream
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}

uint64_t ggrs_hip_state_bytes(ggrs_world* w) { if (!w) return 0; DeviceGuard dg(w); if (seal(w)) return 0; return w->state_bytes; }
int ggrs_hip_live_state_ptr(ggrs_world* w, void** p) {
    if (!w || !p) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    // keep the header current so an exported block is self-describing
    Header h = header_of(w);
    HIPCHK(w, hipMemcpyAsync(w->live.ptr, &h, 16, hipMemcpyHostToDevice, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    *p = w->live.ptr;
    w->live_handed_out = true;                                      // the caller may read the block after any later tick: it is written by every tick from now on
    return GGRS_OK;
}
int ggrs_hip_adopt_live_state(ggrs_world* w) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = seal_live(w); if (rc) return rc;
    struct { Header h; uint32_t res_cell; } hx;                      // the u32 behind the header: which resource cell the block's producer left current (RES_CELL_IDX_OFF)
    static_assert(offsetof(decltype(hx), res_cell) == RES_CELL_IDX_OFF, "the resource cell index sits right behind struct Header");
    HIPCHK(w, hipMemcpyAsync(&hx, w->live.ptr, sizeof hx, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    const Header h = hx.h;
    if (w->has_resources) w->live.res_cell = hx.res_cell & 1u;
    if (h.len > w->capacity) return w->fail(GGRS_E_INVALID, "adopted state has len %llu > capacity", (unsigned long long)h.len);
    w->len = h.len; w->frame = h.frame;
    w->live.dirty_len = std::max(w->live.dirty_len, w->len);
    ver_touch_all(w); w->live.tag_ok = 0; ver_sync_live(w);        // every column is new
    w->pending_valid = false;
    return GGRS_OK;
}

// ---- STATE DIFF (include/ggrs_hip.h; the kernels: kernels.hpp k_diff_count / k_diff_scan / k_diff_emit) ------------------------------------------------------
// Nothing here is on the tick's path: the generated kernel, its arguments and the request runner are untouched.  A side of the comparison is a packed block, the
// len that cuts its masks, the row versions it holds (none for a foreign block) and which of its two resource cells is current.
namespace {
constexpr uint64_t DIFF_HOST_BYTES = 64u << 10;           // the pinned page a report comes back into: the counters and up to ~1150 entries
struct DiffSide { const uint8_t* ptr = nullptr; uint64_t len = 0; const std::vector<ver_t>* ver = nullptr; uint32_t res_cell = 0; bool live_form = false; };
// what every diff call does first: no uncollected batches, a sealed world with a device, RollbackOrdered::len known, every deferred Save in its slot
int diff_ready(ggrs_world* w) {
    if (!w->pending.empty()) return w->fail(GGRS_E_INVALID, "synchronous request while %zu enqueued batches are uncollected", w->pending.size());
    int rc = seal(w); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to compare");
    rc = len_sync(w); if (rc) return rc;
    return materialise_slots(w);
}
int diff_side(ggrs_world* w, int32_t frame, DiffSide* s) {
    if (frame == GGRS_DIFF_LIVE) {
        const int rc = materialise_live(w); if (rc) return rc;
        s->ptr = w->live.ptr; s->len = w->len; s->ver = &w->live.ver; s->res_cell = w->live.res_cell; s->live_form = true;
        return GGRS_OK;
    }
    for (size_t k = 0; k < w->ring_frame.size(); ++k) if (w->ring_frame[k] == frame) {
        const Block& b = w->slots[w->ring_slot[k]];
        s->ptr = b.ptr; s->len = b.len; s->ver = &b.ver; s->res_cell = b.res_cell; s->live_form = false;
        if (w->dev_spawn) {                                            // spawns decided on the device: the slot's len is what its Save wrote into the header
            HIPCHK(w, hipMemcpyAsync(&s->len, b.ptr, 8, hipMemcpyDeviceToHost, w->stream));
            HIPCHK(w, hipStreamSynchronize(w->stream));
            if (s->len > w->capacity) s->len = w->capacity;
        }
        return GGRS_OK;
    }
    return w->fail(GGRS_E_NO_SNAPSHOT, "no snapshot of frame %d in the ring", frame);
}
// the scratch of a state diff or a query (they never overlap): at least `need` bytes of device memory, grown on demand, and the pinned page reports come back into
int diff_scratch(ggrs_world* w, uint64_t need) {
    if (!w->h_diff) HIPCHK(w, hipHostMalloc((void**)&w->h_diff, DIFF_HOST_BYTES, hipHostMallocDefault));      // pinned: the copy back is one DMA, no staging by the runtime
    if (need > w->diff_bytes) {
        HIPCHK(w, hipStreamSynchronize(w->stream));
        if (w->d_diff) { (void)hipFree(w->d_diff); w->d_diff = nullptr; w->diff_bytes = 0; }
        const uint64_t want = align_up(need + need / 2, 4096);
        HIPCHK(w, hipMalloc((void**)&w->d_diff, want));
        w->diff_bytes = want;
    }
    return GGRS_OK;
}
int diff_run(ggrs_world* w, const DiffSide& A, const DiffSide& B, uint32_t flags, ggrs_diff_report* rep, ggrs_diff_entry* entries, uint32_t max_entries) {
    if (!rep || (max_entries && !entries)) return w->fail(GGRS_E_INVALID, "bad diff arguments (no report, or max_entries without entries)");
    if (flags & ~GGRS_DIFF_TRUST_VERSIONS) return w->fail(GGRS_E_INVALID, "unknown diff flags 0x%x", flags);
    if (w->has_strategy && A.live_form != B.live_form)
        return w->fail(GGRS_E_INVALID, "the live world against a snapshot in a world with a component under a Strategy: live form and Stored form are not comparable");
    const bool trust = (flags & GGRS_DIFF_TRUST_VERSIONS) && A.ver && B.ver && w->knobs.row_versions;
    DiffArgs a; memset(&a, 0, sizeof a);
    a.a = A.ptr; a.b = B.ptr; a.len_a = A.len; a.len_b = B.len; a.off_alive = w->off_alive; a.ts = w->ts;
    uint32_t nq = 0; uint64_t bytes_per_slot_cmp = 0;
    for (uint32_t c = 0; c < w->comps.size(); ++c) {
        const Comp& cc = w->comps[c];
        if (cc.no_rollback) continue;                                  // outside every snapshot
        const uint32_t j = a.n_comps++;
        a.off_present[j] = w->off_present[c]; a.comp_id[j] = (uint8_t)c; a.comp_col0[j] = (uint8_t)nq;
        const bool stored = cc.s_n_words && !A.live_form;              // ring-slot form holds Strategy::Stored
        const uint32_t base = stored ? cc.scol_base : cc.col_base, nw = stored ? cc.s_n_words : cc.n_words, wb = stored ? cc.s_word_bytes : cc.word_bytes;
        for (uint32_t k = 0; k < nw; ++k) {
            const uint32_t col = base + k;
            if (col >= (uint32_t)DIFF_MAX_COLS) return w->fail(GGRS_E_INVALID, "state diff serves worlds of at most %d columns (column_diff is one 64-bit word); component %s reaches column %u", DIFF_MAX_COLS, cc.name.c_str(), col);
            if (trust && !stored && !w->col_ext[col] && (*A.ver)[col] != VER_NONE && (*A.ver)[col] == (*B.ver)[col]) continue;   // the same version of the column on both sides: the same bytes
            a.col_off[nq] = w->col_off[col]; a.col_wb[nq] = (uint8_t)wb; a.col_k[nq] = (uint8_t)col; a.col_word[nq] = (uint8_t)k;
            bytes_per_slot_cmp += wb; ++nq;
        }
        a.comp_ncols[j] = (uint8_t)(nq - a.comp_col0[j]);
    }
    a.n_res = (uint32_t)w->resources.size();
    a.res_off_a = RES_CELL_OFF + A.res_cell * RES_CELL_BYTES; a.res_off_b = RES_CELL_OFF + B.res_cell * RES_CELL_BYTES;
    for (uint32_t r = 0; r < a.n_res && r < GGRS_RESOURCE_MAX; ++r) {
        const ggrs_world::Resource& rr = w->resources[r];
        for (uint32_t i = rr.off / 4; i < (rr.off + rr.word_bytes * rr.n_words + 3) / 4 && i < 16; ++i) a.res_lanes[r] |= (uint16_t)(1u << i);
    }
    const uint64_t span = std::min<uint64_t>(std::max(A.len, B.len), w->cap_pad);
    a.n_units = (uint32_t)((span + 63) / 64);
    const uint64_t cap_e = std::min<uint64_t>(max_entries, (uint64_t)a.n_units * 64u);
    a.max_entries = (uint32_t)cap_e;
    // scratch: counters | entries | any word per unit | entry offset per unit  (counters and entries side by side: a short report comes back in ONE copy)
    const uint64_t o_ent = (uint64_t)DIFF_CNT_WORDS * 8, o_any = align_up(o_ent + cap_e * sizeof(ggrs_diff_entry), ALIGN), o_off = o_any + align_up((uint64_t)a.n_units * 8, ALIGN);
    const uint64_t need = o_off + align_up((uint64_t)a.n_units * 8, ALIGN);
    static_assert((DIFF_CNT_WORDS * 8) % alignof(ggrs_diff_entry) == 0, "the entries sit right behind the counters");
    { const int src = diff_scratch(w, need); if (src) return src; }
    a.cnt = (uint64_t*)w->d_diff; a.unit_any = (uint64_t*)(w->d_diff + o_any); a.unit_off = (uint64_t*)(w->d_diff + o_off); a.entries = (ggrs_diff_entry*)(w->d_diff + o_ent);
    const uint32_t by_size = std::max<uint32_t>(1, (a.n_units + TPB / 64 - 1) / (TPB / 64));
    const uint32_t g = std::min<uint32_t>(by_size, w->diff_max_wgs ? w->diff_max_wgs : 4096u);
    HIPCHK(w, hipMemsetAsync(a.cnt, 0, (size_t)DIFF_CNT_WORDS * 8, w->stream));
    hipLaunchKernelGGL(k_diff_count, dim3(g), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (cap_e) {
        hipLaunchKernelGGL(k_diff_scan, dim3(1), dim3(TPB), 0, w->stream, (const uint64_t*)a.unit_any, a.unit_off, a.n_units);
        HIPCHK(w, hipGetLastError());
        hipLaunchKernelGGL(k_diff_emit, dim3(g), dim3(TPB), 0, w->stream, a);
        HIPCHK(w, hipGetLastError());
    }
    // counters and, where they fit the pinned page, the entries' whole room in one copy; a longer list is fetched once its length is known
    const bool one_copy = o_ent + cap_e * sizeof(ggrs_diff_entry) <= DIFF_HOST_BYTES;
    HIPCHK(w, hipMemcpyAsync(w->h_diff, a.cnt, one_copy ? o_ent + cap_e * sizeof(ggrs_diff_entry) : o_ent, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    const uint64_t* cnt = (const uint64_t*)w->h_diff;
    memset(rep, 0, sizeof *rep);
    rep->len_a = A.len; rep->len_b = B.len; rep->n_entities = cnt[DIFF_CNT_ENT]; rep->n_alive = cnt[DIFF_CNT_ALIVE];
    for (uint32_t c = 0; c < 64; ++c) { rep->n_presence[c] = cnt[DIFF_CNT_PRES + c]; rep->n_value[c] = cnt[DIFF_CNT_VAL + c]; }
    rep->resource_diff = cnt[DIFF_CNT_RES];
    rep->n_entries = (uint32_t)std::min<uint64_t>(rep->n_entities, cap_e);
    if (rep->n_entries && one_copy) memcpy(entries, w->h_diff + o_ent, (size_t)rep->n_entries * sizeof(ggrs_diff_entry));
    else if (rep->n_entries) {
        HIPCHK(w, hipMemcpyAsync(entries, a.entries, (size_t)rep->n_entries * sizeof(ggrs_diff_entry), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(w, hipStreamSynchronize(w->stream));
    }
    ++w->diff_calls; w->diff_last_cols = nq; w->diff_last_bps = (uint32_t)bytes_per_slot_cmp; w->diff_last_units = a.n_units;
    return GGRS_OK;
}
}  // namespace
//   ggrs_dbg_set_diff_grid     at most n workgroups per state-diff launch (0: by size): the report must not depend on it
int ggrs_dbg_set_diff_grid(ggrs_world* w, int n) { if (!w || n < 0 || n > 65535) return -1; w->diff_max_wgs = (uint32_t)n; return 0; }
int ggrs_hip_snapshot_copy(ggrs_world* w, int32_t frame, void* dst_dev) {
    if (!w || !dst_dev) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    if (frame == GGRS_DIFF_LIVE) return w->fail(GGRS_E_INVALID, "snapshot_copy copies a ring frame (the live block: ggrs_hip_live_state_ptr)");
    DiffSide s; rc = diff_side(w, frame, &s); if (rc) return rc;
    HIPCHK(w, hipMemcpyAsync(dst_dev, s.ptr, w->state_bytes, hipMemcpyDeviceToDevice, w->stream));
    // the copy describes itself: RollbackOrdered::len and the current resource cell as the host knows them (what the Save's launch wrote)
    const uint64_t len = s.len; const uint32_t cell = s.res_cell;
    HIPCHK(w, hipMemcpyAsync(dst_dev, &len, 8, hipMemcpyHostToDevice, w->stream));
    if (w->has_resources) HIPCHK(w, hipMemcpyAsync((uint8_t*)dst_dev + RES_CELL_IDX_OFF, &cell, 4, hipMemcpyHostToDevice, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    return GGRS_OK;
}
int ggrs_hip_diff_frames(ggrs_world* w, int32_t frame_a, int32_t frame_b, uint32_t flags, ggrs_diff_report* report, ggrs_diff_entry* entries, uint32_t max_entries) {
    if (!w) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    DiffSide A, B;
    rc = diff_side(w, frame_a, &A); if (rc) return rc;
    rc = diff_side(w, frame_b, &B); if (rc) return rc;
    return diff_run(w, A, B, flags, report, entries, max_entries);
}
int ggrs_hip_diff_block(ggrs_world* w, int32_t frame_a, const void* block_b_dev, uint32_t flags, ggrs_diff_report* report, ggrs_diff_entry* entries, uint32_t max_entries) {
    if (!w) return GGRS_E_INVALID;
    if (!block_b_dev) return w->fail(GGRS_E_INVALID, "diff_block without a block");
    if (flags & GGRS_DIFF_TRUST_VERSIONS) return w->fail(GGRS_E_INVALID, "GGRS_DIFF_TRUST_VERSIONS with a foreign block: it carries no row versions");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    DiffSide A, B;
    rc = diff_side(w, frame_a, &A); if (rc) return rc;
    struct { Header h; uint32_t res_cell; } hx;
    HIPCHK(w, hipMemcpyAsync(&hx, block_b_dev, sizeof hx, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (hx.h.len > w->capacity) return w->fail(GGRS_E_INVALID, "the block's header has len %llu > capacity %llu: not a block of this world", (unsigned long long)hx.h.len, (unsigned long long)w->capacity);
    B.ptr = (const uint8_t*)block_b_dev; B.len = hx.h.len; B.ver = nullptr; B.res_cell = w->has_resources ? (hx.res_cell & 1u) : 0u; B.live_form = false;
    return diff_run(w, A, B, flags, report, entries, max_entries);
}

// ---- CHECKSUM PARTS (include/ggrs_hip.h; the kernels: kernels.hpp k_parts_hash / k_parts_finish, kernel_gen.hpp ggrs_jit_parts) -------------------------------------
// Nothing here is on the tick's path.  The state is one side of a state diff (diff_ready / diff_side above: no batches outstanding, deferred Saves and the lazy live
// block brought up to date, the len of a device-spawn world read from the slot's header).
namespace {
uint32_t parts_count(const ggrs_world* w) { uint32_t n = (uint32_t)w->cks_comp.size() + 1u; for (auto& r : w->resources) n += r.checksummed ? 1u : 0u; return n; }
int parts_run(ggrs_world* w, const DiffSide& S, ggrs_parts_report* rep, ggrs_checksum_part* parts, uint32_t max_parts) {
    const uint32_t n_cks = (uint32_t)w->cks_comp.size(), n_parts = parts_count(w);
    if (!rep || !parts) return w->fail(GGRS_E_INVALID, "bad checksum_parts arguments (no report, or no parts array)");
    if (max_parts < n_parts) return w->fail(GGRS_E_INVALID, "max_parts %u is below the world's %u checksum parts (%u components, the entities, %u resources)", max_parts, n_parts, n_cks, n_parts - n_cks - 1u);
    if (!S.live_form) for (uint32_t c : w->cks_comp) {
        const Comp& cc = w->comps[c];
        if (cc.s_n_words) return w->fail(GGRS_E_INVALID, "checksum parts of a snapshot in a world where checksummed component %s is under a Strategy: the slot holds Stored words, the checksum is over live words (GGRS_DIFF_LIVE is served)", cc.name.c_str());
        if (cc.no_rollback) return w->fail(GGRS_E_INVALID, "checksum parts of a snapshot in a world where checksummed component %s is not registered for rollback: no snapshot holds it (GGRS_DIFF_LIVE is served)", cc.name.c_str());
    }
    // a world with a user-written hasher: the hashing kernel is generated at the first call and comes through the module caches
    if (w->custom_hashers && !w->cparts_fn) {
        const std::string keep = w->err;
        const int rc = jit_cached(w, jit_parts_source(w), &w->cparts_fn, &w->cparts_entry, &w->cparts_origin, "ggrs_jit_parts", "generated checksum-parts kernel");
        if (rc != GGRS_OK) {
            const std::string why = w->err.substr(0, 300);
            w->cparts_fn = nullptr; w->err = keep;
            return w->fail(GGRS_E_INVALID, "checksum parts of a world with a user-written hasher need its generated kernel: %s%s", hiprtc_for(w).lib ? "" : "no run-time compiler and no cached code object -- ", why.c_str());
        }
        ++w->cparts_builds;
    }
    if (!w->h_cparts) HIPCHK(w, hipHostMalloc((void**)&w->h_cparts, PARTS_OUT_BYTES, hipHostMallocDefault));
    if (!w->d_cparts) HIPCHK(w, hipMalloc((void**)&w->d_cparts, PARTS_SCRATCH_BYTES));
    PartsArgs a; memset(&a, 0, sizeof a);
    a.state = S.ptr; a.words = reinterpret_cast<const PartsWord*>(w->d_units); a.acc = reinterpret_cast<unsigned long long*>(w->d_cparts);
    a.len = std::min<uint64_t>(S.len, w->capacity); a.off_alive = w->off_alive; a.n_cks = n_cks;
    a.n_units = (uint32_t)((a.len + 63) / 64);
    for (uint32_t k = 0; k < n_cks; ++k) { a.off_present[k] = w->cks_args.off_present[k]; a.n_words[k] = w->cks_args.n_units[k]; a.word_base[k] = w->cks_args.unit_base[k]; }
    PartsFinArgs f; memset(&f, 0, sizeof f);
    f.acc = a.acc; f.out = w->d_cparts + PARTS_OUT_OFF; f.len = a.len; f.n_cks = n_cks;
    f.res_cell = S.ptr + RES_CELL_OFF + S.res_cell * RES_CELL_BYTES;
    for (uint32_t k = 0; k < n_cks; ++k) f.comp_id[k] = w->cks_comp[k];
    for (uint32_t r = 0; r < w->resources.size(); ++r) {
        const ggrs_world::Resource& rr = w->resources[r];
        if (!rr.checksummed) continue;
        const uint32_t j = f.n_res++;
        f.res_id[j] = r; f.res_wb[j] = (uint8_t)rr.word_bytes; f.res_nw[j] = (uint8_t)rr.cks_words.size();
        for (uint32_t i = 0; i < rr.cks_words.size() && i < (uint32_t)MAX_UNITS; ++i) f.res_off[j][i] = (uint8_t)(rr.off + rr.cks_words[i] * rr.word_bytes);
    }
    HIPCHK(w, hipMemsetAsync(a.acc, 0, PARTS_ACC_BYTES, w->stream));
    if (w->cparts_timed) { for (hipEvent_t& e : w->cparts_ev) if (!e) HIPCHK(w, hipEventCreate(&e)); HIPCHK(w, hipEventRecord(w->cparts_ev[0], w->stream)); }
    if (a.n_units) {
        const uint32_t by_size = (a.n_units + PARTS_WAVES - 1) / PARTS_WAVES;
        const uint32_t g = std::max<uint32_t>(1, std::min<uint32_t>(by_size, w->cparts_max_wgs ? w->cparts_max_wgs : 2048u));
        if (w->custom_hashers) {
            void* params[] = {&a};
            HIPCHK(w, hipModuleLaunchKernel(w->cparts_fn, g, 1, 1, TPB, 1, 1, 0, w->stream, params, nullptr));
        } else {
            hipLaunchKernelGGL(k_parts_hash, dim3(g), dim3(TPB), 0, w->stream, a);
            HIPCHK(w, hipGetLastError());
        }
    }
    if (w->cparts_timed) HIPCHK(w, hipEventRecord(w->cparts_ev[1], w->stream));
    hipLaunchKernelGGL(k_parts_finish, dim3(1), dim3(TPB), 0, w->stream, f);
    HIPCHK(w, hipGetLastError());
    if (w->cparts_timed) HIPCHK(w, hipEventRecord(w->cparts_ev[2], w->stream));
    // the report and the parts: one copy into pinned host memory
    HIPCHK(w, hipMemcpyAsync(w->h_cparts, f.out, PARTS_OUT_PARTS + (size_t)n_parts * sizeof(ggrs_checksum_part), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (w->cparts_timed) for (int k = 0; k < 2; ++k) { float ms = 0; HIPCHK(w, hipEventElapsedTime(&ms, w->cparts_ev[k], w->cparts_ev[k + 1])); w->cparts_us[k] = (double)ms * 1e3; }
    memcpy(rep, w->h_cparts, sizeof *rep);
    memcpy(parts, w->h_cparts + PARTS_OUT_PARTS, (size_t)n_parts * sizeof(ggrs_checksum_part));
    ++w->cparts_calls;
    return GGRS_OK;
}
}  // namespace
//   ggrs_dbg_set_parts_grid    at most n workgroups for the hashing launch of a checksum-parts call (0: by size): the report must not depend on it
int ggrs_dbg_set_parts_grid(ggrs_world* w, int n) { if (!w || n < 0 || n > 65535) return -1; w->cparts_max_wgs = (uint32_t)n; return 0; }
//   ggrs_dbg_parts_launch_us   enable != 0: every later checksum-parts call puts HIP events around its two launches; us_out (may be NULL) receives what the hashing
//                              launch and k_parts_finish of the last timed call took by themselves, in microseconds (scripts/bench_checksum_parts.py)
int ggrs_dbg_parts_launch_us(ggrs_world* w, int enable, double* us_out) {
    if (!w) return -1;
    w->cparts_timed = enable != 0;
    if (us_out) { us_out[0] = w->cparts_us[0]; us_out[1] = w->cparts_us[1]; }
    return 0;
}
int ggrs_hip_checksum_parts(ggrs_world* w, int32_t frame, ggrs_parts_report* report, ggrs_checksum_part* parts, uint32_t max_parts) {
    if (!w) return GGRS_E_INVALID;
    if (w->layout_only) return w->fail(GGRS_E_INVALID, "a layout-only world has no state to take checksum parts of");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    DiffSide S; rc = diff_side(w, frame, &S); if (rc) return rc;
    return parts_run(w, S, report, parts, max_parts);
}
int ggrs_hip_checksum_parts_block(ggrs_world* w, const void* block_dev, ggrs_parts_report* report, ggrs_checksum_part* parts, uint32_t max_parts) {
    if (!w) return GGRS_E_INVALID;
    if (w->layout_only) return w->fail(GGRS_E_INVALID, "a layout-only world has no state to take checksum parts of");
    if (!block_dev) return w->fail(GGRS_E_INVALID, "checksum_parts_block without a block");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    struct { Header h; uint32_t res_cell; } hx;
    HIPCHK(w, hipMemcpyAsync(&hx, block_dev, sizeof hx, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (hx.h.len > w->capacity) return w->fail(GGRS_E_INVALID, "the block's header has len %llu > capacity %llu: not a block of this world", (unsigned long long)hx.h.len, (unsigned long long)w->capacity);
    DiffSide S; S.ptr = (const uint8_t*)block_dev; S.len = hx.h.len; S.ver = nullptr; S.res_cell = w->has_resources ? (hx.res_cell & 1u) : 0u; S.live_form = false;
    return parts_run(w, S, report, parts, max_parts);
}

// ---- QUERY (include/ggrs_hip.h; the kernels: kernels.hpp k_query_match / k_diff_scan / k_query_emit) ------------------------------------------------------------------
// Nothing here is on the tick's path.  The state is one side of a state diff (diff_ready / diff_side above); the scratch is the state diff's.
namespace {
// what needs no state: the desc against the world's components.  *with: with_mask and the components of the fetched words
int query_check(ggrs_world* w, const ggrs_query_desc* d, uint64_t* with) {
    if (!d) return w->fail(GGRS_E_INVALID, "query without a desc");
    if (d->n_words > GGRS_QUERY_MAX_WORDS) return w->fail(GGRS_E_INVALID, "a query fetches at most %d words, not %u", GGRS_QUERY_MAX_WORDS, d->n_words);
    if (d->flags & ~GGRS_QUERY_SLOTS) return w->fail(GGRS_E_INVALID, "unknown query flags 0x%x", d->flags);
    const uint64_t known = w->comps.size() >= 64 ? ~0ull : (1ull << w->comps.size()) - 1ull;
    if ((d->with_mask | d->without_mask) & ~known) return w->fail(GGRS_E_INVALID, "a query filter names a component the world does not have (with 0x%llx, without 0x%llx, %zu components)", (unsigned long long)d->with_mask, (unsigned long long)d->without_mask, w->comps.size());
    uint64_t wm = d->with_mask;
    for (uint32_t k = 0; k < d->n_words; ++k) {
        const ggrs_query_word& q = d->words[k];
        if (q.comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "fetched word %u names component %u: the world has %zu", k, q.comp, w->comps.size());
        if (q.word >= w->comps[q.comp].n_words) return w->fail(GGRS_E_INVALID, "fetched word %u names word %u of component %s, which has %u", k, q.word, w->comps[q.comp].name.c_str(), w->comps[q.comp].n_words);
        wm |= 1ull << q.comp;
    }
    if (wm & d->without_mask) return w->fail(GGRS_E_INVALID, "a query names the same component With (or fetches it) and Without (0x%llx): nothing can match", (unsigned long long)(wm & d->without_mask));
    if ((d->flags & GGRS_QUERY_SLOTS) && w->capacity > (1ull << 32)) return w->fail(GGRS_E_INVALID, "GGRS_QUERY_SLOTS writes 32-bit slots: the world's capacity %llu exceeds 2^32", (unsigned long long)w->capacity);
    *with = wm;
    return GGRS_OK;
}
void query_layout(const ggrs_world* w, const ggrs_query_desc* d, uint64_t max_rows, ggrs_query_layout* out) {
    memset(out, 0, sizeof *out);
    uint64_t off = 0;
    for (uint32_t k = 0; k < d->n_words; ++k) {
        const uint32_t wb = w->comps[d->words[k].comp].word_bytes;
        out->col_off[k] = off; out->word_bytes[k] = wb;
        off = align_up(off + max_rows * wb, 256);
    }
    if (d->flags & GGRS_QUERY_SLOTS) { out->slots_off = off; off = align_up(off + max_rows * 4u, 256); }
    out->total_bytes = off;
}
// what a desc that passed query_check may not ask of a ring frame or a block (ring-slot form)
int query_check_snapshot(ggrs_world* w, const ggrs_query_desc* d, uint64_t with) {
    for (uint32_t c = 0; c < w->comps.size(); ++c) if (((with | d->without_mask) >> c) & 1ull) {
        if (w->comps[c].no_rollback) return w->fail(GGRS_E_INVALID, "a query of a snapshot names component %s, which is not registered for rollback: no snapshot holds it (GGRS_DIFF_LIVE is served)", w->comps[c].name.c_str());
    }
    for (uint32_t k = 0; k < d->n_words; ++k) {
        const Comp& cc = w->comps[d->words[k].comp];
        if (cc.s_n_words) return w->fail(GGRS_E_INVALID, "a query of a snapshot fetches words of component %s, which is under a Strategy: the slot holds Stored words (GGRS_DIFF_LIVE is served)", cc.name.c_str());
    }
    return GGRS_OK;
}
// the launches' arguments for a checked desc over state S (the scratch pointers are the caller's)
void query_args(const ggrs_world* w, const DiffSide& S, const ggrs_query_desc* d, uint64_t with, void* out_dev, uint64_t max_rows, QueryArgs& a) {
    ggrs_query_layout lay; query_layout(w, d, max_rows, &lay);
    memset(&a, 0, sizeof a);
    a.state = S.ptr; a.out = (uint8_t*)out_dev; a.len = std::min<uint64_t>(S.len, w->capacity); a.max_rows = max_rows; a.off_alive = w->off_alive; a.slots_off = lay.slots_off;
    for (uint32_t c = 0; c < w->comps.size() && c < 64u; ++c) {
        const bool wi = (with >> c) & 1ull, wo = (d->without_mask >> c) & 1ull;
        if (!wi && !wo) continue;
        if (wo) a.without |= 1u << a.n_masks;
        a.off_mask[a.n_masks++] = w->off_present[c];
    }
    a.n_words = d->n_words; a.slots = (d->flags & GGRS_QUERY_SLOTS) ? 1u : 0u;
    for (uint32_t k = 0; k < d->n_words; ++k) {
        const uint32_t col = w->comps[d->words[k].comp].col_base + d->words[k].word;
        a.col_off[k] = w->col_off[col]; a.col_ts[k] = w->col_ts[col]; a.col_wb[k] = (uint8_t)w->col_wb[col]; a.out_off[k] = lay.col_off[k];
    }
    a.n_units = (uint32_t)((a.len + 63) / 64);
}
int query_run(ggrs_world* w, const DiffSide& S, const ggrs_query_desc* d, void* out_dev, uint64_t max_rows, ggrs_query_report* rep) {
    uint64_t with = 0;
    int rc = query_check(w, d, &with); if (rc) return rc;
    if (!rep) return w->fail(GGRS_E_INVALID, "query without a report");
    if (!out_dev && max_rows) return w->fail(GGRS_E_INVALID, "query with max_rows %llu and no output buffer", (unsigned long long)max_rows);
    if (!S.live_form) { rc = query_check_snapshot(w, d, with); if (rc) return rc; }
    QueryArgs a; query_args(w, S, d, with, out_dev, max_rows, a);
    memset(rep, 0, sizeof *rep);
    rep->len = S.len;
    // scratch: match word per unit + the sentinel | first row per unit + the total
    const uint64_t words = (uint64_t)a.n_units + 1u, o_off = align_up(words * 8, ALIGN);
    rc = diff_scratch(w, o_off + align_up(words * 8, ALIGN)); if (rc) return rc;
    a.unit_match = (uint64_t*)w->d_diff; a.unit_off = (uint64_t*)(w->d_diff + o_off);
    const uint32_t cap = w->query_max_wgs ? w->query_max_wgs : 4096u;
    const uint32_t g_match = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((words + TPB - 1) / TPB), cap));
    const uint32_t g_emit = std::max<uint32_t>(1, std::min<uint32_t>((a.n_units + TPB / 64 - 1) / (TPB / 64), cap));
    const bool emit = max_rows && a.n_units && (a.n_words || a.slots);
    if (w->query_timed) { for (hipEvent_t& e : w->query_ev) if (!e) HIPCHK(w, hipEventCreate(&e)); HIPCHK(w, hipEventRecord(w->query_ev[0], w->stream)); }
    hipLaunchKernelGGL(k_query_match, dim3(g_match), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[1], w->stream));
    hipLaunchKernelGGL(k_diff_scan, dim3(1), dim3(TPB), 0, w->stream, (const uint64_t*)a.unit_match, a.unit_off, (uint32_t)words);
    HIPCHK(w, hipGetLastError());
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[2], w->stream));
    if (emit) {
        hipLaunchKernelGGL(k_query_emit, dim3(g_emit), dim3(TPB), 0, w->stream, a);
        HIPCHK(w, hipGetLastError());
    }
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[3], w->stream));
    // the count: the scan's word behind the last unit, one copy into the pinned page
    HIPCHK(w, hipMemcpyAsync(w->h_diff, a.unit_off + a.n_units, 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (w->query_timed) for (int k = 0; k < 3; ++k) { float ms = 0; HIPCHK(w, hipEventElapsedTime(&ms, w->query_ev[k], w->query_ev[k + 1])); w->query_us[k] = (double)ms * 1e3; }
    rep->n_matched = *(const uint64_t*)w->h_diff;
    rep->n_rows = std::min<uint64_t>(rep->n_matched, max_rows);
    ++w->query_calls; w->query_last_words = a.n_words; w->query_last_masks = a.n_masks + 1u; w->query_last_units = a.n_units;
    return GGRS_OK;
}
}  // namespace
//   ggrs_dbg_set_query_grid    at most n workgroups per query launch (0: by size): the output must not depend on it
int ggrs_dbg_set_query_grid(ggrs_world* w, int n) { if (!w || n < 0 || n > 65535) return -1; w->query_max_wgs = (uint32_t)n; return 0; }
//   ggrs_dbg_query_launch_us   enable != 0: every later query call puts HIP events around its launches; us_out (may be NULL) receives what the match, scan and emit
//                              launches of the last timed call took by themselves, in microseconds (scripts/bench_query.py)
int ggrs_dbg_query_launch_us(ggrs_world* w, int enable, double* us_out) {
    if (!w) return -1;
    w->query_timed = enable != 0;
    if (us_out) for (int k = 0; k < 3; ++k) us_out[k] = w->query_us[k];
    return 0;
}
int ggrs_hip_query_layout(ggrs_world* w, const ggrs_query_desc* desc, uint64_t max_rows, ggrs_query_layout* out) {
    if (!w) return GGRS_E_INVALID;
    if (!out) return w->fail(GGRS_E_INVALID, "query_layout without a layout to fill");
    uint64_t with = 0;
    const int rc = query_check(w, desc, &with); if (rc) return rc;
    if (max_rows > (1ull << 48)) return w->fail(GGRS_E_INVALID, "query_layout for %llu rows", (unsigned long long)max_rows);
    query_layout(w, desc, max_rows, out);
    return GGRS_OK;
}
int ggrs_hip_query(ggrs_world* w, int32_t frame, const ggrs_query_desc* desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report) {
    if (!w) return GGRS_E_INVALID;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to query");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    DiffSide S; rc = diff_side(w, frame, &S); if (rc) return rc;
    return query_run(w, S, desc, out_dev, max_rows, report);
}
// inspection: the index of a ring frame or of the live world, built exactly as ahead of a request group (publish, then the k_ix_* launches) and copied out.  The
// view and the index are rebuilt ahead of every group that reads them, so overwriting them here disturbs nothing.
int ggrs_hip_peer_index_read(ggrs_world* w, int32_t frame, uint32_t* start, uint32_t* slots, uint64_t* n_indexed) {
    if (!w) return GGRS_E_INVALID;
    if (!w->peer_index.on) return w->fail(GGRS_E_INVALID, "peer_index_read: the world has no peer index (ggrs_hip_register_peer_index)");
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to index");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    DiffSide S; rc = diff_side(w, frame, &S); if (rc) return rc;
    const ggrs_world::PeerIndex& ix = w->peer_index;
    std::vector<uint32_t> st((size_t)ix.n_buckets + 1, 0);
    if (S.len) {
        GgrsJitArgs j; memset(&j, 0, offsetof(GgrsJitArgs, inputs));
        rc = publish_peers(w, S.ptr, S.len, j); if (rc) return rc;
        HIPCHK(w, hipMemcpyAsync(st.data(), ix.d_start, st.size() * 4, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(w, hipStreamSynchronize(w->stream));
        if (st.back() > S.len) return w->fail(GGRS_E_HIP, "peer index: %u indexed slots in a state of len %llu", st.back(), (unsigned long long)S.len);
        if (slots && st.back()) {
            HIPCHK(w, hipMemcpyAsync(slots, ix.d_slots, (size_t)st.back() * 4, hipMemcpyDeviceToHost, w->stream));
            HIPCHK(w, hipStreamSynchronize(w->stream));
        }
    }
    if (start) memcpy(start, st.data(), st.size() * 4);
    if (n_indexed) *n_indexed = st.back();
    return GGRS_OK;
}
int ggrs_hip_query_block(ggrs_world* w, const void* block_dev, const ggrs_query_desc* desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report) {
    if (!w) return GGRS_E_INVALID;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to query");
    if (!block_dev) return w->fail(GGRS_E_INVALID, "query_block without a block");
    DeviceGuard dg(w);
    int rc = diff_ready(w); if (rc) return rc;
    Header h;
    HIPCHK(w, hipMemcpyAsync(&h, block_dev, sizeof h, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (h.len > w->capacity) return w->fail(GGRS_E_INVALID, "the block's header has len %llu > capacity %llu: not a block of this world", (unsigned long long)h.len, (unsigned long long)w->capacity);
    DiffSide S; S.ptr = (const uint8_t*)block_dev; S.len = h.len; S.ver = nullptr; S.res_cell = 0; S.live_form = false;
    return query_run(w, S, desc, out_dev, max_rows, report);
}

// ---- SORTED QUERY (include/ggrs_hip.h; the kernels: kernels.hpp k_query_match / k_diff_scan as they are, k_sort_rows, k_sort_rekey + the k_ix_* passes or k_sort_small,
// k_sort_emit) -----------------------------------------------------------------------------------------------------------------------------------------------------
// Nothing here is on the tick's path.  Both descs are judged before the device is looked at: whether the state is the live world is known from the frame number.
namespace {
// *with gains the keys' components (a key's component counts as named in with_mask)
int sort_check(ggrs_world* w, const ggrs_query_desc* d, const ggrs_sort_desc* s, bool live, const void* out_dev, uint64_t max_rows, const ggrs_query_report* rep, uint64_t* with) {
    int rc = query_check(w, d, with); if (rc) return rc;
    if (!s) return w->fail(GGRS_E_INVALID, "sorted query without a sort desc");
    if (s->n_keys == 0) return w->fail(GGRS_E_INVALID, "a sorted query with n_keys 0 has nothing to order by: use ggrs_hip_query");
    if (s->n_keys > GGRS_SORT_MAX_KEYS) return w->fail(GGRS_E_INVALID, "a sorted query takes at most %d keys, not n_keys %u", GGRS_SORT_MAX_KEYS, s->n_keys);
    if (s->flags) return w->fail(GGRS_E_INVALID, "unknown sort flags 0x%x", s->flags);
    for (uint32_t k = 0; k < s->n_keys; ++k) {
        const ggrs_sort_key& q = s->keys[k];
        if ((q.kind & ~GGRS_SORT_DESC) > GGRS_SORT_F) return w->fail(GGRS_E_INVALID, "sort key %u has unknown kind 0x%x (GGRS_SORT_U / _I / _F, | GGRS_SORT_DESC)", k, q.kind);
        if (q.comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "sort key %u names component %u: the world has %zu", k, q.comp, w->comps.size());
        const Comp& cc = w->comps[q.comp];
        if (q.word >= cc.n_words) return w->fail(GGRS_E_INVALID, "sort key %u names word %u of component %s, which has %u", k, q.word, cc.name.c_str(), cc.n_words);
        if ((q.kind & ~GGRS_SORT_DESC) == GGRS_SORT_F && cc.word_bytes < 4) return w->fail(GGRS_E_INVALID, "sort key %u is GGRS_SORT_F on the %u-byte words of component %s: 4- and 8-byte words only", k, cc.word_bytes, cc.name.c_str());
        if ((d->without_mask >> q.comp) & 1ull) return w->fail(GGRS_E_INVALID, "sort key %u names component %s, which is also in without_mask: nothing can match", k, cc.name.c_str());
        if (!live && cc.s_n_words) return w->fail(GGRS_E_INVALID, "sort key %u names a word of component %s, which is under a Strategy: a snapshot holds Stored words (GGRS_DIFF_LIVE is served)", k, cc.name.c_str());
        if (!live && cc.no_rollback) return w->fail(GGRS_E_INVALID, "sort key %u names a word of component %s, which is not registered for rollback: no snapshot holds it (GGRS_DIFF_LIVE is served)", k, cc.name.c_str());
        *with |= 1ull << q.comp;
    }
    if (!live) { rc = query_check_snapshot(w, d, *with); if (rc) return rc; }
    if (w->capacity > (1ull << 32)) return w->fail(GGRS_E_INVALID, "a sorted query orders 32-bit slots: the world's capacity %llu exceeds 2^32", (unsigned long long)w->capacity);
    if (!rep) return w->fail(GGRS_E_INVALID, "sorted query without a report");
    if (!out_dev && max_rows) return w->fail(GGRS_E_INVALID, "sorted query with max_rows %llu and no output buffer", (unsigned long long)max_rows);
    return GGRS_OK;
}
int sort_run(ggrs_world* w, const DiffSide& S, const ggrs_query_desc* d, const ggrs_sort_desc* sd, uint64_t with, void* out_dev, uint64_t max_rows, ggrs_query_report* rep) {
    QueryArgs a; query_args(w, S, d, with, out_dev, max_rows, a);
    SortArgs s; memset(&s, 0, sizeof s);
    s.state = S.ptr;
    for (uint32_t k = sd->n_keys; k-- > 0;) {                          // stages, least significant first: keys[n_keys-1] .. keys[0], an 8-byte word's low half before its high half
        const ggrs_sort_key& q = sd->keys[k];
        const uint32_t col = w->comps[q.comp].col_base + q.word, wb = w->col_wb[col];
        for (uint32_t half = 0; half < (wb == 8 ? 2u : 1u); ++half) {
            SortStage& st = s.st[s.n_stages++];
            st.col_off = w->col_off[col]; st.col_ts = w->col_ts[col]; st.passes = wb >= 4 ? 4u : wb; st.wb = (uint8_t)wb;
            st.kind = (uint8_t)(q.kind & ~GGRS_SORT_DESC); st.desc = (q.kind & GGRS_SORT_DESC) ? 1 : 0; st.half = (uint8_t)half;
        }
    }
    memset(rep, 0, sizeof *rep);
    rep->len = S.len;
    // scratch: match word per unit + the sentinel | first row per unit + the total | key 0 | key 1 | val 0 | val 1 | the digit-major table (256 words per tile)
    const uint64_t words = (uint64_t)a.n_units + 1u, o_off = align_up(words * 8, ALIGN), tiles_max = std::max<uint64_t>(1, (a.len + IX_TILE - 1) / IX_TILE);
    const uint64_t pair_bytes = align_up(tiles_max * IX_TILE * 4u, ALIGN), o_pair = o_off + align_up(words * 8, ALIGN), o_hist = o_pair + 4 * pair_bytes;
    static_assert(ALIGN % 16 == 0, "k_ix_scan loads the table as uint4");
    int rc = diff_scratch(w, o_hist + align_up(tiles_max * 256u * 4u, ALIGN)); if (rc) return rc;
    a.unit_match = (uint64_t*)w->d_diff; a.unit_off = (uint64_t*)(w->d_diff + o_off);
    for (uint32_t i = 0; i < 2; ++i) { s.key[i] = (uint32_t*)(w->d_diff + o_pair + i * pair_bytes); s.val[i] = (uint32_t*)(w->d_diff + o_pair + (2 + i) * pair_bytes); }
    uint32_t* const hist = (uint32_t*)(w->d_diff + o_hist);
    const uint32_t cap = w->query_max_wgs ? w->query_max_wgs : 4096u;
    const uint32_t g_match = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((words + TPB - 1) / TPB), cap));
    const uint32_t g_unit = std::max<uint32_t>(1, std::min<uint32_t>((a.n_units + TPB / 64 - 1) / (TPB / 64), cap));
    const bool timed = w->sort_timed;
    if (timed) { for (hipEvent_t& e : w->sort_ev) if (!e) HIPCHK(w, hipEventCreate(&e)); HIPCHK(w, hipEventRecord(w->sort_ev[0], w->stream)); }
    hipLaunchKernelGGL(k_query_match, dim3(g_match), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (timed) HIPCHK(w, hipEventRecord(w->sort_ev[1], w->stream));
    hipLaunchKernelGGL(k_diff_scan, dim3(1), dim3(TPB), 0, w->stream, (const uint64_t*)a.unit_match, a.unit_off, (uint32_t)words);
    HIPCHK(w, hipGetLastError());
    if (timed) HIPCHK(w, hipEventRecord(w->sort_ev[2], w->stream));
    // the count, before anything else is launched: the radix kernels take n and n_tiles by value
    HIPCHK(w, hipMemcpyAsync(w->h_diff, a.unit_off + a.n_units, 8, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    const uint64_t n = *(const uint64_t*)w->h_diff;
    if (n > a.len) return w->fail(GGRS_E_HIP, "sorted query: %llu matches in a state of len %llu", (unsigned long long)n, (unsigned long long)a.len);
    rep->n_matched = n;
    rep->n_rows = std::min<uint64_t>(n, max_rows);
    uint32_t launches = 2;
    const bool sorts = n && max_rows && (a.n_words || a.slots);          // a desc that fetches no word and no slot writes nothing: a count, whatever max_rows is
    if (sorts) {
        s.n = n;
        hipLaunchKernelGGL(k_sort_rows, dim3(g_unit), dim3(TPB), 0, w->stream, a, s);
        HIPCHK(w, hipGetLastError());
        ++launches;
        if (timed) HIPCHK(w, hipEventRecord(w->sort_ev[3], w->stream));
        uint32_t cur = 0;
        if (n <= IX_TILE && !w->sort_force_large) {
            hipLaunchKernelGGL(k_sort_small, dim3(1), dim3(IX_TPB), 0, w->stream, s);
            HIPCHK(w, hipGetLastError());
            ++launches;
            for (uint32_t g = 0; g < s.n_stages; ++g) cur ^= s.st[g].passes & 1u;
        } else {
            const uint32_t n_tiles = (uint32_t)((n + IX_TILE - 1) / IX_TILE);
            const uint32_t g_row = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((n + TPB - 1) / TPB), cap));
            for (uint32_t g = 0; g < s.n_stages; ++g) {
                if (g) { hipLaunchKernelGGL(k_sort_rekey, dim3(g_row), dim3(TPB), 0, w->stream, s, g, cur); HIPCHK(w, hipGetLastError()); ++launches; }
                for (uint32_t p = 0; p < s.st[g].passes; ++p, cur ^= 1u) {
                    IxArgs x; memset(&x, 0, sizeof x);
                    x.key_in = s.key[cur]; x.val_in = s.val[cur]; x.key_out = s.key[cur ^ 1u]; x.val_out = s.val[cur ^ 1u]; x.hist = hist;
                    x.n = n; x.n_tiles = n_tiles; x.shift = 8u * p;
                    hipLaunchKernelGGL((k_ix_hist<false>), dim3(n_tiles), dim3(IX_TPB), 0, w->stream, x);
                    hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(IX_SCAN_TPB), 0, w->stream, hist, n_tiles);
                    hipLaunchKernelGGL((k_ix_scatter<false>), dim3(n_tiles), dim3(IX_TPB), 0, w->stream, x);
                    HIPCHK(w, hipGetLastError());
                    launches += 3;
                }
            }
        }
        if (timed) HIPCHK(w, hipEventRecord(w->sort_ev[4], w->stream));
        const uint32_t g_out = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((rep->n_rows + TPB - 1) / TPB), cap));
        hipLaunchKernelGGL(k_sort_emit, dim3(g_out), dim3(TPB), 0, w->stream, a, (const uint32_t*)s.val[cur], rep->n_rows);
        HIPCHK(w, hipGetLastError());
        ++launches;
        if (timed) HIPCHK(w, hipEventRecord(w->sort_ev[5], w->stream));
        HIPCHK(w, hipStreamSynchronize(w->stream));
    }
    if (timed) {
        const int last = sorts ? 5 : 2;
        for (int k = 0; k < 5; ++k) w->sort_us[k] = 0;
        for (int k = 0; k < last; ++k) { float ms = 0; HIPCHK(w, hipEventElapsedTime(&ms, w->sort_ev[k], w->sort_ev[k + 1])); w->sort_us[k] = (double)ms * 1e3; }
    }
    ++w->sort_calls; w->sort_last_stages = s.n_stages; w->sort_last_launches = launches;
    return GGRS_OK;
}
}  // namespace
//   ggrs_dbg_set_sort_form             0: one workgroup sorts a result of at most IX_TILE rows in one launch (k_sort_small), 1: always the large form; the output must not depend on it
int ggrs_dbg_set_sort_form(ggrs_world* w, int form) { if (!w || form < 0 || form > 1) return -1; w->sort_force_large = form == 1; return 0; }
//   ggrs_dbg_sorted_query_launch_us    enable != 0: every later sorted query puts HIP events around its phases; us_out (may be NULL) receives what match, scan, the host's
//                                      read of the count together with the rows launch (one figure, mostly the wait), the stages and the emit of the last timed call took, in microseconds (scripts/bench_sorted_query.py)
int ggrs_dbg_sorted_query_launch_us(ggrs_world* w, int enable, double* us_out) {
    if (!w) return -1;
    w->sort_timed = enable != 0;
    if (us_out) for (int k = 0; k < 5; ++k) us_out[k] = w->sort_us[k];
    return 0;
}
int ggrs_hip_query_sorted(ggrs_world* w, int32_t frame, const ggrs_query_desc* query_desc, const ggrs_sort_desc* sort_desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report) {
    if (!w) return GGRS_E_INVALID;
    uint64_t with = 0;
    int rc = sort_check(w, query_desc, sort_desc, frame == GGRS_DIFF_LIVE, out_dev, max_rows, report, &with); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to query");
    DeviceGuard dg(w);
    rc = diff_ready(w); if (rc) return rc;
    DiffSide S; rc = diff_side(w, frame, &S); if (rc) return rc;
    return sort_run(w, S, query_desc, sort_desc, with, out_dev, max_rows, report);
}
int ggrs_hip_query_sorted_block(ggrs_world* w, const void* block_dev, const ggrs_query_desc* query_desc, const ggrs_sort_desc* sort_desc, void* out_dev, uint64_t max_rows, ggrs_query_report* report) {
    if (!w) return GGRS_E_INVALID;
    if (!block_dev) return w->fail(GGRS_E_INVALID, "query_sorted_block without a block");
    uint64_t with = 0;
    int rc = sort_check(w, query_desc, sort_desc, false, out_dev, max_rows, report, &with); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to query");
    DeviceGuard dg(w);
    rc = diff_ready(w); if (rc) return rc;
    Header h;
    HIPCHK(w, hipMemcpyAsync(&h, block_dev, sizeof h, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (h.len > w->capacity) return w->fail(GGRS_E_INVALID, "the block's header has len %llu > capacity %llu: not a block of this world", (unsigned long long)h.len, (unsigned long long)w->capacity);
    DiffSide S; S.ptr = (const uint8_t*)block_dev; S.len = h.len; S.ver = nullptr; S.res_cell = 0; S.live_form = false;
    return sort_run(w, S, query_desc, sort_desc, with, out_dev, max_rows, report);
}

// ---- DELTA (include/ggrs_hip.h; the kernels: kernels.hpp k_delta_match_masks / k_delta_match_values, then k_diff_scan / k_query_emit as they are) --------------------
// Nothing here is on the tick's path.  The two states are sides of a state diff (diff_ready / diff_side above); the scratch, the grid cap and the launch timer are
// the query's.  The descriptor is judged before the device is looked at: which side is the live world is known from the frame numbers alone.
namespace {
const char* const DELTA_KINDS[] = {"CHANGED", "ADDED", "REMOVED", "DESPAWNED"};
int delta_check(ggrs_world* w, const ggrs_delta_desc* d, bool new_live, bool old_live, bool old_block, const void* out_dev, uint64_t max_rows, const ggrs_delta_report* rep, uint64_t* with) {
    if (!d) return w->fail(GGRS_E_INVALID, "delta without a desc");
    int rc = query_check(w, &d->q, with); if (rc) return rc;
    if (d->kind > GGRS_DELTA_DESPAWNED) return w->fail(GGRS_E_INVALID, "unknown delta kind %u", d->kind);
    if (d->flags & ~GGRS_DELTA_TRUST_VERSIONS) return w->fail(GGRS_E_INVALID, "unknown delta flags 0x%x", d->flags);
    const bool base_live = d->kind <= GGRS_DELTA_ADDED ? new_live : old_live;
    if (!base_live) { rc = query_check_snapshot(w, &d->q, *with); if (rc) return rc; }
    const uint64_t known = w->comps.size() >= 64 ? ~0ull : (1ull << w->comps.size()) - 1ull;
    if (d->changed_mask & ~known) return w->fail(GGRS_E_INVALID, "changed_mask 0x%llx names a component the world does not have (%zu components)", (unsigned long long)d->changed_mask, w->comps.size());
    if (d->kind == GGRS_DELTA_DESPAWNED && d->changed_mask) return w->fail(GGRS_E_INVALID, "changed_mask 0x%llx in a delta DESPAWNED: it asks about no component and must be 0", (unsigned long long)d->changed_mask);
    if (d->kind != GGRS_DELTA_DESPAWNED && !d->changed_mask) return w->fail(GGRS_E_INVALID, "a delta %s with an empty changed_mask asks about no component", DELTA_KINDS[d->kind]);
    uint32_t ncols = 0;
    for (uint32_t c = 0; c < w->comps.size() && c < 64u; ++c) if ((d->changed_mask >> c) & 1ull) {
        const Comp& cc = w->comps[c];
        if (cc.no_rollback && !(new_live && old_live)) return w->fail(GGRS_E_INVALID, "changed_mask names component %s, which is not registered for rollback: no snapshot holds it", cc.name.c_str());
        if (d->kind != GGRS_DELTA_CHANGED) continue;
        if (cc.s_n_words && !cc.no_rollback && new_live != old_live)
            return w->fail(GGRS_E_INVALID, "a delta CHANGED of component %s, which is under a Strategy, between the live world and a snapshot: live form and Stored form are not comparable", cc.name.c_str());
        ncols += (cc.s_n_words && !cc.no_rollback && !new_live) ? cc.s_n_words : cc.n_words;
    }
    if (ncols > (uint32_t)DIFF_MAX_COLS) return w->fail(GGRS_E_INVALID, "a delta CHANGED compares at most %d columns, not %u", DIFF_MAX_COLS, ncols);
    if ((d->flags & GGRS_DELTA_TRUST_VERSIONS) && old_block) return w->fail(GGRS_E_INVALID, "GGRS_DELTA_TRUST_VERSIONS with a foreign block: it carries no row versions");
    if (!rep) return w->fail(GGRS_E_INVALID, "delta without a report");
    if (!out_dev && max_rows) return w->fail(GGRS_E_INVALID, "delta with max_rows %llu and no output buffer", (unsigned long long)max_rows);
    return GGRS_OK;
}
int delta_run(ggrs_world* w, const DiffSide& N, const DiffSide& O, const ggrs_delta_desc* d, uint64_t with, void* out_dev, uint64_t max_rows, ggrs_delta_report* rep) {
    const bool new_based = d->kind <= GGRS_DELTA_ADDED;
    const DiffSide& S = new_based ? N : O;                              // the base side: the filter and the fetched words are taken there
    const DiffSide& X = new_based ? O : N;
    QueryArgs qa; query_args(w, S, &d->q, with, out_dev, max_rows, qa);
    DeltaArgs a; memset(&a, 0, sizeof a);
    a.base = S.ptr; a.other = X.ptr; a.len_base = qa.len; a.len_other = std::min<uint64_t>(X.len, w->capacity); a.off_alive = w->off_alive;
    a.n_units = qa.n_units; a.n_masks = qa.n_masks; a.without = qa.without; a.kind = d->kind;
    for (uint32_t j = 0; j < qa.n_masks; ++j) a.off_mask[j] = qa.off_mask[j];
    const bool trust = (d->flags & GGRS_DELTA_TRUST_VERSIONS) && N.ver && O.ver && w->knobs.row_versions;
    uint32_t nq = 0;
    for (uint32_t c = 0; c < w->comps.size() && c < 64u; ++c) if ((d->changed_mask >> c) & 1ull) {
        const Comp& cc = w->comps[c];
        const uint32_t j = a.n_comps++;
        a.off_present[j] = w->off_present[c]; a.comp_col0[j] = (uint8_t)nq;
        if (d->kind != GGRS_DELTA_CHANGED) continue;
        const bool stored = cc.s_n_words && !cc.no_rollback && !N.live_form;    // ring-slot form holds Strategy::Stored (delta_check: both sides have one form)
        const uint32_t base = stored ? cc.scol_base : cc.col_base, nw = stored ? cc.s_n_words : cc.n_words;
        bool same = trust && !stored;                                  // the same version of every column and of the presence row on both sides: the same words
        if (same) { const uint32_t p = ver_presence(w, c); same = (*N.ver)[p] != VER_NONE && (*N.ver)[p] == (*O.ver)[p]; }
        for (uint32_t k = 0; k < nw && same; ++k) same = !w->col_ext[base + k] && (*N.ver)[base + k] != VER_NONE && (*N.ver)[base + k] == (*O.ver)[base + k];
        if (same) continue;                                            // (its masks are still compared: added needs no column)
        for (uint32_t k = 0; k < nw; ++k, ++nq) { a.col_off[nq] = w->col_off[base + k]; a.col_ts[nq] = w->col_ts[base + k]; a.col_wb[nq] = (uint8_t)w->col_wb[base + k]; }
        a.comp_ncols[j] = (uint8_t)(nq - a.comp_col0[j]);
    }
    memset(rep, 0, sizeof *rep);
    rep->len_new = N.len; rep->len_old = O.len;
    // scratch: match word per unit + the sentinel | first row per unit + the total
    const uint64_t words = (uint64_t)a.n_units + 1u, o_off = align_up(words * 8, ALIGN);
    int rc = diff_scratch(w, o_off + align_up(words * 8, ALIGN)); if (rc) return rc;
    a.unit_match = qa.unit_match = (uint64_t*)w->d_diff; qa.unit_off = (uint64_t*)(w->d_diff + o_off);
    const uint32_t cap = w->query_max_wgs ? w->query_max_wgs : 4096u;
    const uint32_t g_lane = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((words + TPB - 1) / TPB), cap));
    const uint32_t g_wave = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)((words + TPB / 64 - 1) / (TPB / 64)), cap));
    const uint32_t g_emit = std::max<uint32_t>(1, std::min<uint32_t>((a.n_units + TPB / 64 - 1) / (TPB / 64), cap));
    const bool emit = max_rows && qa.n_units && (qa.n_words || qa.slots);
    if (w->query_timed) { for (hipEvent_t& e : w->query_ev) if (!e) HIPCHK(w, hipEventCreate(&e)); HIPCHK(w, hipEventRecord(w->query_ev[0], w->stream)); }
    if (d->kind == GGRS_DELTA_CHANGED) hipLaunchKernelGGL(k_delta_match_values, dim3(g_wave), dim3(TPB), 0, w->stream, a);
    else hipLaunchKernelGGL(k_delta_match_masks, dim3(g_lane), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[1], w->stream));
    hipLaunchKernelGGL(k_diff_scan, dim3(1), dim3(TPB), 0, w->stream, (const uint64_t*)qa.unit_match, qa.unit_off, (uint32_t)words);
    HIPCHK(w, hipGetLastError());
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[2], w->stream));
    if (emit) {
        hipLaunchKernelGGL(k_query_emit, dim3(g_emit), dim3(TPB), 0, w->stream, qa);
        HIPCHK(w, hipGetLastError());
    }
    if (w->query_timed) HIPCHK(w, hipEventRecord(w->query_ev[3], w->stream));
    // the count: the scan's word behind the last unit.  The rows beyond old's len (NEW-based kinds, new longer than old): all rows less those below it, which the
    // scan word and the match word of unit len_old >> 6 give -- no counter, no atomic
    uint64_t* const h = (uint64_t*)w->h_diff;
    const uint64_t cut = a.len_other >> 6;
    const bool tail = new_based && a.len_other < a.len_base;           // (then cut < n_units)
    HIPCHK(w, hipMemcpyAsync(h, qa.unit_off + a.n_units, 8, hipMemcpyDeviceToHost, w->stream));
    if (tail) {
        HIPCHK(w, hipMemcpyAsync(h + 1, qa.unit_off + cut, 8, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(w, hipMemcpyAsync(h + 2, qa.unit_match + cut, 8, hipMemcpyDeviceToHost, w->stream));
    }
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (w->query_timed) for (int k = 0; k < 3; ++k) { float ms = 0; HIPCHK(w, hipEventElapsedTime(&ms, w->query_ev[k], w->query_ev[k + 1])); w->query_us[k] = (double)ms * 1e3; }
    rep->n_matched = h[0];
    rep->n_rows = std::min<uint64_t>(rep->n_matched, max_rows);
    if (tail) rep->n_beyond_old_len = rep->n_matched - (h[1] + (uint64_t)__builtin_popcountll(h[2] & ((1ull << (a.len_other & 63u)) - 1ull)));
    ++w->delta_calls; w->delta_last_kind = d->kind; w->delta_last_cols = nq; w->delta_last_comps = a.n_comps; w->delta_last_units = a.n_units;
    return GGRS_OK;
}
}  // namespace
int ggrs_hip_delta_frames(ggrs_world* w, int32_t frame_new, int32_t frame_old, const ggrs_delta_desc* desc, void* out_dev, uint64_t max_rows, ggrs_delta_report* report) {
    if (!w) return GGRS_E_INVALID;
    uint64_t with = 0;
    int rc = delta_check(w, desc, frame_new == GGRS_DIFF_LIVE, frame_old == GGRS_DIFF_LIVE, false, out_dev, max_rows, report, &with); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no states to take a delta of");
    DeviceGuard dg(w);
    rc = diff_ready(w); if (rc) return rc;
    DiffSide N, O;
    rc = diff_side(w, frame_new, &N); if (rc) return rc;
    rc = diff_side(w, frame_old, &O); if (rc) return rc;
    return delta_run(w, N, O, desc, with, out_dev, max_rows, report);
}
int ggrs_hip_delta_block(ggrs_world* w, int32_t frame_new, const void* block_old_dev, const ggrs_delta_desc* desc, void* out_dev, uint64_t max_rows, ggrs_delta_report* report) {
    if (!w) return GGRS_E_INVALID;
    if (!block_old_dev) return w->fail(GGRS_E_INVALID, "delta_block without a block");
    uint64_t with = 0;
    int rc = delta_check(w, desc, frame_new == GGRS_DIFF_LIVE, false, true, out_dev, max_rows, report, &with); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no states to take a delta of");
    DeviceGuard dg(w);
    rc = diff_ready(w); if (rc) return rc;
    DiffSide N, O;
    rc = diff_side(w, frame_new, &N); if (rc) return rc;
    Header h;
    HIPCHK(w, hipMemcpyAsync(&h, block_old_dev, sizeof h, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (h.len > w->capacity) return w->fail(GGRS_E_INVALID, "the block's header has len %llu > capacity %llu: not a block of this world", (unsigned long long)h.len, (unsigned long long)w->capacity);
    O.ptr = (const uint8_t*)block_old_dev; O.len = h.len; O.ver = nullptr; O.res_cell = 0; O.live_form = false;
    return delta_run(w, N, O, desc, with, out_dev, max_rows, report);
}

// ---- SCATTER (include/ggrs_hip.h; the kernels: kernels.hpp k_scatter_check / k_scatter_apply) ------------------------------------------------------------------------
// Nothing here is on the tick's path.  The target is the live block; the input buffer's layout is the query's (query_layout); the record and the report travel as
// the query's count does (diff_scratch and its pinned page).  The host's bookkeeping is what ggrs_hip_upload_word / _insert_component / _remove_component / _despawn
// do per call, done once -- and only when the rows were applied.
namespace {
constexpr uint32_t SCATTER_MAX_WGS = 2048;                 // 8 workgroups per CU: full occupancy; beyond it a lane takes several rows (grid-stride)
// what needs no state: the desc against the world's components.  *masks: the components whose presence word the apply launch reads (WRITE) or edits (INSERT, REMOVE)
int scatter_check(ggrs_world* w, const ggrs_scatter_desc* d, const void* in_dev, uint64_t stride_rows, uint64_t n_rows, const ggrs_scatter_report* rep, uint64_t* masks) {
    static const char* const OPS[] = {"WRITE", "INSERT", "REMOVE", "DESPAWN"};
    if (!d) return w->fail(GGRS_E_INVALID, "scatter without a desc");
    if (d->op > GGRS_SCATTER_DESPAWN) return w->fail(GGRS_E_INVALID, "unknown scatter op %u", d->op);
    if (d->flags) return w->fail(GGRS_E_INVALID, "unknown scatter flags 0x%x", d->flags);
    const bool carries = d->op <= GGRS_SCATTER_INSERT;
    const uint64_t known = w->comps.size() >= 64 ? ~0ull : (1ull << w->comps.size()) - 1ull;
    if (carries && d->n_words == 0) return w->fail(GGRS_E_INVALID, "a scatter %s names no word", OPS[d->op]);
    if (d->n_words > GGRS_QUERY_MAX_WORDS) return w->fail(GGRS_E_INVALID, "a scatter carries at most %d words, not %u", GGRS_QUERY_MAX_WORDS, d->n_words);
    if (!carries && d->n_words) return w->fail(GGRS_E_INVALID, "a scatter %s carries no words, not %u", OPS[d->op], d->n_words);
    if (d->op != GGRS_SCATTER_REMOVE && d->comp_mask) return w->fail(GGRS_E_INVALID, "comp_mask 0x%llx in a scatter %s: it names what REMOVE removes and is 0 otherwise", (unsigned long long)d->comp_mask, OPS[d->op]);
    if (d->op == GGRS_SCATTER_REMOVE && !d->comp_mask) return w->fail(GGRS_E_INVALID, "a scatter REMOVE with an empty comp_mask removes nothing");
    if (d->comp_mask & ~known) return w->fail(GGRS_E_INVALID, "a scatter REMOVE names a component the world does not have (comp_mask 0x%llx, %zu components)", (unsigned long long)d->comp_mask, w->comps.size());
    uint64_t m = d->comp_mask;
    uint32_t named[MAX_COMPS] = {0};
    for (uint32_t k = 0; k < d->n_words; ++k) {
        const ggrs_query_word& q = d->words[k];
        if (q.comp >= w->comps.size()) return w->fail(GGRS_E_INVALID, "scatter word %u names component %u: the world has %zu", k, q.comp, w->comps.size());
        if (q.word >= w->comps[q.comp].n_words) return w->fail(GGRS_E_INVALID, "scatter word %u names word %u of component %s, which has %u", k, q.word, w->comps[q.comp].name.c_str(), w->comps[q.comp].n_words);
        for (uint32_t j = 0; j < k; ++j) if (d->words[j].comp == q.comp && d->words[j].word == q.word)
            return w->fail(GGRS_E_INVALID, "scatter words %u and %u both name word %u of component %s", j, k, q.word, w->comps[q.comp].name.c_str());
        m |= 1ull << q.comp; ++named[q.comp];
    }
    if (d->op == GGRS_SCATTER_INSERT) for (uint32_t c = 0; c < w->comps.size(); ++c) if (named[c] && named[c] != w->comps[c].n_words)
        return w->fail(GGRS_E_INVALID, "a scatter INSERT names %u of the %u words of component %s: an inserted component brings every word (defaults are out of scope)", named[c], w->comps[c].n_words, w->comps[c].name.c_str());
    if (!in_dev && n_rows) return w->fail(GGRS_E_INVALID, "scatter of %llu rows and no input buffer", (unsigned long long)n_rows);
    if (n_rows > stride_rows) return w->fail(GGRS_E_INVALID, "scatter of %llu rows from a buffer laid out for %llu", (unsigned long long)n_rows, (unsigned long long)stride_rows);
    if (stride_rows > (1ull << 48)) return w->fail(GGRS_E_INVALID, "scatter from a buffer laid out for %llu rows", (unsigned long long)stride_rows);
    if (!rep) return w->fail(GGRS_E_INVALID, "scatter without a report");
    if (w->capacity > (1ull << 32)) return w->fail(GGRS_E_INVALID, "scatter rows carry 32-bit slots: the world's capacity %llu exceeds 2^32", (unsigned long long)w->capacity);
    *masks = m;
    return GGRS_OK;
}
}  // namespace
//   ggrs_dbg_scatter_launch_us  enable != 0: every later scatter call puts HIP events around its launches; us_out (may be NULL) receives what the check and apply
//                               launches of the last timed call took by themselves, in microseconds (scripts/bench_scatter.py)
int ggrs_dbg_scatter_launch_us(ggrs_world* w, int enable, double* us_out) {
    if (!w) return -1;
    w->scatter_timed = enable != 0;
    if (us_out) { us_out[0] = w->scatter_us[0]; us_out[1] = w->scatter_us[1]; }
    return 0;
}
int ggrs_hip_scatter(ggrs_world* w, const ggrs_scatter_desc* desc, const void* in_dev, uint64_t stride_rows, uint64_t n_rows, ggrs_scatter_report* report) {
    if (!w) return GGRS_E_INVALID;
    uint64_t masks = 0;
    int rc = scatter_check(w, desc, in_dev, stride_rows, n_rows, report, &masks); if (rc) return rc;
    if (w->layout_only) return w->fail(GGRS_E_NO_DEVICE, "a layout-only world has no state to scatter into");
    DeviceGuard dg(w);
    if (w->dev_spawn && !w->pending.empty())
        return w->fail(GGRS_E_INVALID, "scatter into a world whose systems spawn on the device while %zu enqueued batches are uncollected: its len is not known to the host", w->pending.size());
    rc = seal_live(w); if (rc) return rc;
    memset(report, 0, sizeof *report);
    report->len = w->len; report->n_rows = n_rows; report->first_bad_row = ~0ull;
    if (n_rows == 0) return GGRS_OK;
    // the input buffer's layout is a query's: the same words, the slots behind them
    ggrs_query_desc qd; memset(&qd, 0, sizeof qd);
    qd.n_words = desc->n_words; qd.flags = GGRS_QUERY_SLOTS;
    for (uint32_t k = 0; k < desc->n_words; ++k) qd.words[k] = desc->words[k];
    ggrs_query_layout lay; query_layout(w, &qd, stride_rows, &lay);
    ScatterArgs a; memset(&a, 0, sizeof a);
    a.state = w->live.ptr; a.in = (const uint8_t*)in_dev; a.len = std::min<uint64_t>(w->len, w->capacity); a.n_rows = n_rows; a.off_alive = w->off_alive; a.slots_off = lay.slots_off;
    a.op = desc->op; a.n_words = desc->n_words;
    if (desc->op != GGRS_SCATTER_DESPAWN) for (uint32_t c = 0; c < w->comps.size() && c < 64u; ++c) if ((masks >> c) & 1ull) a.off_mask[a.n_masks++] = w->off_present[c];
    for (uint32_t k = 0; k < desc->n_words; ++k) {
        const uint32_t col = w->comps[desc->words[k].comp].col_base + desc->words[k].word;
        a.col_off[k] = w->col_off[col]; a.col_ts[k] = w->col_ts[col]; a.col_wb[k] = (uint8_t)w->col_wb[col]; a.in_off[k] = lay.col_off[k];
    }
    rc = diff_scratch(w, (uint64_t)SCAT_REC_WORDS * 8u); if (rc) return rc;
    a.rec = reinterpret_cast<unsigned long long*>(w->d_diff);
    const uint32_t cap = w->query_max_wgs ? w->query_max_wgs : SCATTER_MAX_WGS;
    const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_rows + TPB - 1) / TPB, cap));
    // the record: every count 0, the lowest bad row (kept as its complement) none
    HIPCHK(w, hipMemsetAsync(a.rec, 0, (size_t)SCAT_REC_WORDS * 8u, w->stream));
    if (w->scatter_timed) { for (hipEvent_t& e : w->scatter_ev) if (!e) HIPCHK(w, hipEventCreate(&e)); HIPCHK(w, hipEventRecord(w->scatter_ev[0], w->stream)); }
    hipLaunchKernelGGL(k_scatter_check, dim3(g), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (w->scatter_timed) HIPCHK(w, hipEventRecord(w->scatter_ev[1], w->stream));
    hipLaunchKernelGGL(k_scatter_apply, dim3(g), dim3(TPB), 0, w->stream, a);
    HIPCHK(w, hipGetLastError());
    if (w->scatter_timed) HIPCHK(w, hipEventRecord(w->scatter_ev[2], w->stream));
    HIPCHK(w, hipMemcpyAsync(w->h_diff, a.rec, (size_t)SCAT_REC_WORDS * 8u, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipStreamSynchronize(w->stream));
    if (w->scatter_timed) for (int k = 0; k < 2; ++k) { float ms = 0; HIPCHK(w, hipEventElapsedTime(&ms, w->scatter_ev[k], w->scatter_ev[k + 1])); w->scatter_us[k] = (double)ms * 1e3; }
    const uint64_t* r = (const uint64_t*)w->h_diff;
    ++w->scatter_calls; w->scatter_last_rows = n_rows; w->scatter_last_op = desc->op; w->scatter_last_words = desc->n_words;
    if (r[SCAT_BAD]) {                                              // the apply launch returned at once: not a byte, not a version, not a tag bit has changed
        report->first_bad_row = ~r[SCAT_FIRST_BAD];
        return w->fail(GGRS_E_INVALID, "scatter rows must be strictly ascending slots below len %llu: %llu of %llu rows are not, first_bad_row %llu",
                       (unsigned long long)w->len, (unsigned long long)r[SCAT_BAD], (unsigned long long)n_rows, (unsigned long long)~r[SCAT_FIRST_BAD]);
    }
    report->n_dead = r[SCAT_DEAD]; report->n_absent = r[SCAT_ABSENT]; report->n_applied = n_rows - r[SCAT_DEAD] - r[SCAT_ABSENT];
    for (uint32_t k = 0; k < desc->n_words; ++k) {                  // written columns (WRITE, INSERT)
        const uint32_t col = w->comps[desc->words[k].comp].col_base + desc->words[k].word;
        ver_touch(w, col); live_tags_lost(w, col);
    }
    if (desc->op == GGRS_SCATTER_INSERT || desc->op == GGRS_SCATTER_REMOVE)
        for (uint32_t c = 0; c < w->comps.size() && c < 64u; ++c) if ((masks >> c) & 1ull) ver_touch(w, ver_presence(w, c));
    ver_sync_live(w);
    w->pending_valid = false;
    return GGRS_OK;
}

// Which kernel serves this world's request lists right now, on what kind of arena, and the state of the run-time
// compiler -- `key=value` lines (NUL-terminated, truncated to cap).  Nothing here is needed to USE the library: it is what an
// operator reads when a world is slower than expected (e.g. libhiprtc.so missing from a deployment image).
int ggrs_hip_world_kernel_info(ggrs_world* w, char* buf, uint64_t cap, uint64_t* needed) {
    if (!w || (!buf && cap)) return GGRS_E_INVALID;
    std::string s;
    char line[768];
    auto add = [&](const char* k, const std::string& v) { snprintf(line, sizeof line, "%s=%s\n", k, v.c_str()); s += line; };
    add("sealed", w->sealed ? "1" : "0");
    {
        uint32_t n_ready = 0, n_building = 0, n_failed = 0; std::string why;
        for (auto& t : w->spec_tab) {
            const int st = t.spec ? t.spec->state.load(std::memory_order_acquire) : 0;
            n_ready += st == 2 && t.spec->coop != 0; n_building += st == 1;
            if (st == 3 || (st == 2 && t.spec->coop == 0)) { ++n_failed; why = t.spec->why; }     // (coop 0: built, but the device does not hold a device-spawn world's grid of it)
        }
        std::string v = !w->knobs.jit_specialise_after ? "off (GGRS_JIT_SPECIALISE_AFTER=0)"
                      : n_ready ? "ready (" + std::to_string(n_ready) + " of " + std::to_string(w->spec_tab.size()) + " group shapes seen run on kernels compiled for them" +
                                  (n_building ? ", 1 building" : "") + (n_failed ? ", " + std::to_string(n_failed) + " failed: " + why : "") + ")"
                      : n_building ? "building" : n_failed ? "failed: " + why : "none yet";
        for (char& ch : v) if (ch == '\n') ch = ' ';
        add("specialised_kernel", v);
    }
    add("arena", !w->sealed ? "none" : (!w->own_arena ? "caller-provided" : "paged (hipMalloc)"));
    add("arena_bytes", std::to_string(w->arena_bytes));
    {
        Hiprtc& r = hiprtc_for(w);
        add("hiprtc", r.lib ? "loaded" : ("missing: " + r.why));
    }
    add("generated_kernel", w->jit_fn ? "ok" : w->jit_status);
    if (w->jit_fn) add("generated_kernel_origin", w->jit_origin);
    std::string k;
    const uint64_t cover = std::max(w->len, w->live.dirty_len);
    if (!w->sealed) k = "unknown (not sealed)";
    else if (w->gen_ok) k = "ggrs_jit_tick (generated for this world; one workgroup per 256 slots)";
    else k = "per-request kernels (k_copy_state, one launch per system)";
    add("request_group_kernel", k);
    if (w->sealed && w->gen_ok) {
        // who folds the per-workgroup checksum rows of a plain (no batch) request group of this size
        const uint32_t g = std::max<uint32_t>(1, (uint32_t)((cover + 255) / 256));
        const bool ff = w->h_rows && !w->device_results_only && g > (uint32_t)w->knobs.fold_forward_min_wgs;
        const bool host = w->h_rows && !w->device_results_only && !ff;
        std::string f = ff ? "fold-forward: the next launch on the stream folds the rows (k_ff_fold when nothing follows) and the host hashes one value per Save and part; blocking calls: " +
                             std::string(g <= HOST_FOLD_MAX_WGS_BLOCKING && g <= (uint32_t)w->knobs.fold_forward_min_wgs ? "the host folds the rows" : "the launch folds its own rows (self-fold; k_gen_finalize for lists it does not cover)")
                      : host ? (g <= HOST_FOLD_MAX_WGS_BLOCKING ? "the host folds the rows at collect time (blocking calls too)" : "the host folds the rows at collect time (blocking calls: k_gen_finalize)")
                             : "k_gen_finalize";
        add("checksum_fold", f);
        add("kernarg_bytes", std::to_string(w->jl ? w->jl->bytes : 0));
        add("lazy_live_block", !lazy_live_possible(w) ? "off (live-only state, a component under a Strategy, a handed-out pointer, results on the device, or per-request launches)"
                                   : cover <= JIT_NT_MIN_SLOTS ? "off (the world fits the caches: the live block's bytes are not what bounds the launch)"
                                   : "on after " + std::to_string(LAZY_LIVE_STREAK) + " lists in a row that open with a LoadGameState: " + std::to_string(w->lazy_skips) + " lists left it unwritten, " +
                                     std::to_string(w->lazy_materialised) + " materialised on demand");
        add("deferred_saves", std::string(lazy_live_possible(w) && !w->has_strategy && defer_saves_on(w) ? "on" : "off") + " (rollback groups of the same sessions store their first Save only): " +
                              std::to_string(w->saves_deferred) + " Saves deferred, " + std::to_string(w->slots_materialised) + " ring slots materialised on demand");
        add("depth_parallel_roles", std::to_string(w->dp_groups) + " request groups so far split their Saves and the live block over roles (blockIdx.y)");
        add("group_caps", std::to_string(w->cap_saves) + " saves / " + std::to_string(w->cap_steps) + " steps");
        if (w->has_peers) add("peer_view", std::to_string(w->peer_view.n_cols) + " linear columns + visibility words, published from the group's source block ahead of every request group that holds an AdvanceWorld (" +
                                           std::to_string(w->peer_view.publishes) + " publishes so far)");
        if (w->peer_index.on) add("peer_index", std::to_string(w->peer_index.n_buckets) + " buckets over word " + std::to_string(w->peer_index.word) + " of component " + w->comps[w->peer_index.comp].name +
                                                ", rebuilt from the view behind every publish (" + std::to_string(w->peer_index.builds) + " builds, " + std::to_string(w->peer_index.launches) + " launches so far)");
        if (w->has_commands) add("command_bindings", std::to_string(__builtin_popcountll(w->cmd_mut_comps)) + " components a system may insert or remove: their presence bits are registers of the generated kernel, "
                                                     "their mask words are rebuilt per Save, and every AdvanceWorld gives their masks and columns fresh row versions");
        if (w->has_resources) add("device_resources", std::to_string(w->resources.size()) + " resources, " + std::to_string(res_total_bytes(w)) + " bytes: wave-uniform registers of the generated kernel, loaded from the source block's current cell "
                                                      "(two cells per block; the live block's is cell " + std::to_string(w->live.res_cell) + "), stored with every snapshot's header");
        if (w->has_reduces) add("reduce_inbox", std::to_string(w->rd_inbox.stripes) + " stripes of 64 bytes laid out like a resource cell, " + std::to_string(w->rd_inbox.n_words) + " reduced words holding the ops' identities, folded into the live block's current resource cell right behind every request group that holds an AdvanceWorld (" +
                                                std::to_string(w->rd_inbox.applies) + " applies so far)");
        if (w->has_remote) add("remote_inbox", "one u32 per slot, " + std::to_string(w->rx_inbox.n_comps) + " remotely commanded components (bit 0 despawn, bits 1 + 2k / 2 + 2k insert / remove of component k), zeros whenever no group-and-apply pair is in flight, "
                                               "applied to the live block's masks and columns right behind every request group that holds an AdvanceWorld and ahead of the effects (" + std::to_string(w->rx_inbox.applies) + " applies so far)");
        if (w->has_sums) add("sum_partials", std::to_string(w->sum_part.units) + " units of 64 slots, " + std::to_string(w->sum_part.n_words) + " summed words, one 8-byte partial per unit and word stored by the unit's wave, folded by the balanced tree "
                                             "into the live block's current resource cell right behind every request group that holds an AdvanceWorld (" + std::to_string(w->sum_part.applies) + " applies so far)");
        if (w->has_values) add("value_inbox", std::to_string(w->rv_inbox.n_comps) + " value-bound components (one u64 winner word per slot each: the largest key (g + 1) << 40 | (sender slot + 1) of the frame, zeros whenever no group-and-apply pair is in flight), " +
                                              std::to_string(w->rv_inbox.n_bind) + " value bindings (one payload array each: the senders' staged words at their own slots), " + std::to_string(w->rv_inbox.bytes) + " bytes allocated, applied with the remote inbox (" +
                                              std::to_string(w->rx_inbox.applies) + " applies so far)");
        if (w->has_effects) add("effect_inbox", std::to_string(w->fx_inbox.n_cols) + " linear columns holding the ops' identities, applied to the live block right behind every request group that holds an AdvanceWorld (" +
                                               std::to_string(w->fx_inbox.applies) + " applies so far)");
        add("branch_marker_record_bytes", std::to_string(w->jit_marks ? jit_marks_rec_bytes(w) : 0));      // per retained branch of ggrs_hip_fanout_step_branches (0: the kernel keeps no markers)
        add("branch_marker_records", std::to_string(w->branch_marks_cap));                                 // ... how many are allocated
        bool any_spawn = false;
        for (auto& sd : w->systems) any_spawn |= sd.kind == GGRS_SYS_PARTICLES_SPAWN || sd.kind == GGRS_SYS_SPAWN_CUSTOM;
        if (w->dev_spawn && jit_dev_stream(w)) { char t[256]; snprintf(t, sizeof t, "one streamed launch per request group: %u workgroups take tiles by ticket, children numbered by decoupled look-back (%d VGPRs, %d SGPRs)", w->sp_tiles, w->sp_regs, w->sp_sregs); add("device_spawn", t); }
        else if (w->dev_spawn) { char t[160]; snprintf(t, sizeof t, "one cooperative launch per request group: %u workgroups, %d resident per CU x %d CUs (%d VGPRs, %d SGPRs)", 8u * ((w->sp_tiles + 7u) / 8u), w->sp_per_cu, w->n_cu, w->sp_regs, w->sp_sregs); add("device_spawn", t); }
        if (any_spawn) add("spawn_system", w->jit_spawn_sys >= 0 ? "runs inside the request group (rows appended by the group's launch)" : "ends the request group (its own launches)");
    }
    add("blocking_wait", w->knobs.spin_wait_us > 0 ? "polls k_gen_finalize's completion tags when that kernel ends the list (" + std::to_string(w->spin_hits) + " calls so far, " +
                                                      std::to_string(w->spin_misses) + " fell back to the stream wait), else hipStreamSynchronize"
                                                    : "hipStreamSynchronize (GGRS_SPIN_WAIT_US=0)");
    add("slots_covered", std::to_string(cover));
    if (w->diff_calls) add("state_diff", std::to_string(w->diff_calls) + " calls; the last one compared " + std::to_string(w->diff_last_cols) + " columns (" + std::to_string(w->diff_last_bps) +
                                         " bytes per slot and side) and " + std::to_string(w->plan.n_masks) + " masks over " + std::to_string(w->diff_last_units) + " units of 64 slots");
    if (w->query_calls) add("query", std::to_string(w->query_calls) + " calls; the last one fetched " + std::to_string(w->query_last_words) + " words and read " + std::to_string(w->query_last_masks) +
                                     " masks over " + std::to_string(w->query_last_units) + " units of 64 slots");
    if (w->delta_calls) add("delta", std::to_string(w->delta_calls) + " calls; the last one was kind " + std::to_string(w->delta_last_kind) + " over " + std::to_string(w->delta_last_comps) + " components, compared " +
                                     std::to_string(w->delta_last_cols) + " columns over " + std::to_string(w->delta_last_units) + " units of 64 slots");
    if (w->scatter_calls) add("scatter", std::to_string(w->scatter_calls) + " calls; the last one was op " + std::to_string(w->scatter_last_op) + " over " + std::to_string(w->scatter_last_rows) + " rows of " +
                                         std::to_string(w->scatter_last_words) + " words");
    if (w->cparts_calls) add("checksum_parts", std::to_string(w->cparts_calls) + " calls; hashing kernel " + (w->custom_hashers ? "ggrs_jit_parts (generated: the world has a user-written hasher; module from " + w->cparts_origin + ", " +
                                             std::to_string(w->cparts_builds) + " built or loaded by this world)" : std::string("k_parts_hash (static)")));
    add("row_versions", w->knobs.row_versions ? "on" : "off (GGRS_ROW_VERSIONS=0)");
    add("value_tags", !w->sealed ? "unknown (not sealed)" : w->vtags ? "on: a Save skips the columns whose 64 values per unit the destination already holds (" + std::to_string(w->prof_skipped) + " bytes not stored in profiled launches; the ids' numbering has started over " + std::to_string(w->tag_wraps) + " times)"
                                 : "off (the world's steady Save moves less than " + std::to_string(VTAGS_MIN_BYTES >> 20) + " MB, or row versions are off)");
    if (needed) *needed = s.size() + 1;
    if (buf && cap) { const uint64_t n = std::min<uint64_t>(cap, s.size() + 1); memcpy(buf, s.c_str(), n); buf[n - 1] = 0; }
    return GGRS_OK;
}

int ggrs_hip_profile_enable(ggrs_world* w, int on) {
    if (!w) return GGRS_E_INVALID;
    w->prof = on != 0;
    if (on) { DeviceGuard dg(w);
              for (auto& e : w->prof_events) { w->prof_pool.push_back(e.a); w->prof_pool.push_back(e.b); } w->prof_events.clear();
              while (w->prof_pool.size() < 512) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) break; w->prof_pool.push_back(e); }     // (outside whatever the caller times)
              for (int i = 0; i < (int)GGRS_KERNEL_CLASSES; ++i) { w->prof_ms[i] = 0; w->prof_n[i] = 0; w->prof_bytes[i] = 0; w->prof_launch_us[i].clear(); }
              w->prof_skipped = 0; if (w->d_skip) { (void)hipStreamSynchronize(w->stream); (void)hipMemset(w->d_skip, 0, 8); } }
    return GGRS_OK;
}
// drains the recorded event pairs into the per-class totals and per-launch lists
static int profile_drain(ggrs_world* w) {
    HIPCHK(w, hipStreamSynchronize(w->stream));
    for (auto& e : w->prof_events) {
        float ms = 0; (void)hipEventElapsedTime(&ms, e.a, e.b);
        w->prof_ms[e.cls] += ms; w->prof_n[e.cls] += 1;
        if (w->prof_launch_us[e.cls].size() < 65536) w->prof_launch_us[e.cls].push_back(ms * 1e3f);
        if (w->prof_pool.size() < 4096) { w->prof_pool.push_back(e.a); w->prof_pool.push_back(e.b); } else { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    }
    w->prof_events.clear();
    // value tags: what the profiled launches did NOT store comes off the bytes they were asked to move
    if (w->d_skip) {
        uint64_t skipped = 0;
        HIPCHK(w, hipMemcpy(&skipped, w->d_skip, 8, hipMemcpyDeviceToHost));
        if (skipped) { HIPCHK(w, hipMemset(w->d_skip, 0, 8)); w->prof_bytes[GGRS_KERNEL_TICK] -= std::min<uint64_t>(skipped, w->prof_bytes[GGRS_KERNEL_TICK]); w->prof_skipped += skipped; }
    }
    return GGRS_OK;
}
int ggrs_hip_profile_read_launches(ggrs_world* w, uint32_t cls, float* us_out, uint32_t cap, uint32_t* n_out) {
    if (!w || cls >= GGRS_KERNEL_CLASSES || (!us_out && cap)) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = profile_drain(w); if (rc) return rc;
    const std::vector<float>& v = w->prof_launch_us[cls];
    const uint32_t n = (uint32_t)std::min<size_t>(v.size(), cap);
    if (n) memcpy(us_out, v.data(), (size_t)n * sizeof(float));
    if (n_out) *n_out = (uint32_t)v.size();
    return GGRS_OK;
}
int ggrs_hip_profile_read_bytes(ggrs_world* w, uint64_t* bytes_out) {
    if (!w || !bytes_out) return GGRS_E_INVALID;
    if (w->d_skip && w->sealed) { DeviceGuard dg(w); const int rc = profile_drain(w); if (rc) return rc; }     // value tags: what the launches did not store is known once they ran
    for (int i = 0; i < (int)GGRS_KERNEL_CLASSES; ++i) bytes_out[i] = w->prof_bytes[i];
    return GGRS_OK;
}
int ggrs_hip_profile_read(ggrs_world* w, double* ms_out, uint64_t* launches_out) {
    if (!w || !ms_out || !launches_out) return GGRS_E_INVALID;
    DeviceGuard dg(w);
    int rc = profile_drain(w); if (rc) return rc;
    for (int i = 0; i < (int)GGRS_KERNEL_CLASSES; ++i) { ms_out[i] = w->prof_ms[i]; launches_out[i] = w->prof_n[i]; }
    return GGRS_OK;
}


#include "host_fanout.hpp"
